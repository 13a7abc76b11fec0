"""GPU: a full slot among the first wcap of the key cache also has wide tables, three per 32-bit span of k over digits
of 11, 11 and 10 bits, and a wave whose lanes all have such a key adds 40 table entries, not 48 (the wide items of
fd_ftab_kernel, the 16 extra base points behind fd_keyclaim_kernel's chains and in fd_wbase_kernel, the body dsmf_wide
of fd_dsmh_kernel).

Every case runs small batches forced onto the throughput path (small_batch_max = 0, key_fixed = 2: fixed-base from 4
signatures, key_split = 2) unless it is about pins, in both result-code semantics and through the unfolded and the
carry-folded kernels, each scenario on the GPU once.  The codes always equal the CPU oracle's, and the device's own
counts -- fwide_count: the fixed-base keys whose slot was wide at the walk, the signatures that walked 40 additions;
ffull_count: those that walked without doublings, wide or not -- are each batch's composition, which test_fixtures
checks without a GPU.  The batch helpers are tests/test_gpu_key_split.py's, tests/test_gpu_key_fixed.py's,
tests/test_gpu_key_cache.py's, tests/test_gpu_key_full.py's and tests/test_gpu_key_pin.py's.

A wave that holds a full slot without wide tables walks 48 additions from the byte tables in all its lanes (every
full slot has those), so it counts in ffull_count alone.  With key_wide = 2 the first half of the slots is wide.  On a
fresh context the claims take slots 0, 1, 2, ... in the order the device's atomics decide, so with more keys than
wide slots which keys are wide is the device's choice: the number of wide keys is then exact and the signatures
are bounded by ffull_count's."""
import functools
import hashlib

import numpy as np
import pytest

from tests import test_gpu_key_cache as kc
from tests import test_gpu_key_fixed as kf
from tests import test_gpu_key_full as kfull
from tests import test_gpu_key_pin as kp
from tests import test_gpu_key_split as ks
from tests import torsion

gpu = pytest.mark.gpu

ON, OFF, TESTS = 0, 1, 2
L = ks.L
COMBOS = kfull.COMBOS
W0, W2 = 1024, 520                   # FD_FB_W0, FD_FB_W2 (tests/test_fb_wide_schedule.py checks them against the header)


def _once(f):
    """The suite repeats every GPU test per engine path (tests/conftest.py); this module chooses its engine options
    itself, so a scenario runs on the GPU once and the repeats only find that it passed."""
    return functools.lru_cache(maxsize=None)(f)


def _engine(batches, sem=0, fold=False, max_sig=None, **opts):
    import firedancer_amd as fa
    from firedancer_amd import engine
    fa.load_library()
    o = dict(half=1, small_batch_max=0, key_fixed=TESTS, key_split=2, nofold_max=0 if fold else -1)
    o.update(opts)
    engine.debug_set_opts(**o)
    try:
        return fa.Engine(device=0, max_txn=max(len(b[1]) for b in batches),
                         max_sig=max_sig or max(b[2] for b in batches),
                         max_payload=max(b[0].nbytes for b in batches), semantics=sem)
    finally:
        engine.debug_reset_opts()


# ---- the digit-ends batch: one key, a fixed nonce, messages ground until a digit of k sits at an end ------------

def _scalar(i):
    """The secret scalar of test key i (RFC 8032 5.1.5)"""
    h = bytearray(hashlib.sha512(ks._key(i)[1]).digest()[:32])
    h[0] &= 248
    h[31] &= 127
    h[31] |= 64
    return int.from_bytes(h, "little")


NONCE = int.from_bytes(hashlib.sha512(b"key_wide nonce").digest(), "little") % L


@functools.lru_cache(maxsize=None)
def _r_bytes():
    return torsion.encode(torsion._mul(NONCE, torsion.BASE))


def _wide_digits(k):
    """The 24 wide digits of k: fd_fb_recode's bytes, then fd_fb_wide_split per span, on Python integers"""
    a, carry = [], 0
    for j in range(32):
        v = ((k >> (8 * j)) & 255) + carry
        carry = (v + 128) >> 8
        a.append(v - (carry << 8))
    out = []
    for t in range(8):
        v = sum(a[4 * t + r] << (8 * r) for r in range(4))
        d0 = ((v + 1024) & 2047) - 1024
        v1 = (v - d0) >> 11
        d1 = ((v1 + 1024) & 2047) - 1024
        out += [d0, d1, (v1 - d1) >> 11]
    return out


def _ends(t, r):
    """The ends a digit of table (t, r) can reach: 0, the most negative and the most positive.  k < l < 2^253 bounds
    the top span by 0x10000000 (and by 0x0fffffff plus a carry for every k a hash gives), so its third digit lies in
    [0, 64]"""
    if r < 2:
        return (0, -W0, W0 - 1)
    return (0, 64) if t == 7 else (0, -514, 510)


@functools.lru_cache(maxsize=None)
def _ground():
    """[(message, k)] of at most 72 messages, the first found for every (table, end); and the ends each table meets"""
    pub, rb = ks._key(0)[0], _r_bytes()
    need = {(t, r, e) for t in range(8) for r in range(3) for e in _ends(t, r)}
    picked, i = [], 0
    while need:
        m = b"key_wide digit ends %d" % i
        i += 1
        assert i < 400000, sorted(need)
        k = int.from_bytes(hashlib.sha512(rb + pub + m).digest(), "little") % L
        d = _wide_digits(k)
        hit = {(t, r, d[3 * t + r]) for t in range(8) for r in range(3)} & need
        if hit:
            need -= hit
            picked.append((m, k))
    return picked


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "ends":               # valid signatures S = r + k a mod l under R = [r]B
        a, pub, rb = _scalar(0), ks._key(0)[0], _r_bytes()
        txns = [(m, [(rb + ((NONCE + k * a) % L).to_bytes(32, "little"), pub)]) for m, k in _ground()]
    elif name == "late":             # keys 16..19, ten signatures each
        txns = ks._single([16 + t % 4 for t in range(40)])
    elif name in kfull.OWN:
        return kfull._batch(name)
    else:
        return kp._batch(name)
    return ks._pack(txns)


OWN = ("ends", "late")


@functools.lru_cache(maxsize=None)
def _want(name, sem):
    if name in kfull.OWN:
        return kfull._want(name, sem)
    if name not in OWN:
        return kp._want(name, sem)
    p, d, n = _batch(name)
    return ks._oracle().verify_txns(p, d, n, sem=sem, threads=ks.THREADS)


def _walkers(name):
    if name in OWN:
        return 1 if name == "ends" else 4, _batch(name)[2]
    return kfull._walkers(name)


def _go(eng, name, sem, what=None):
    """Runs the batch, checks its codes, returns (signature codes, ffull_count, fwide_count)"""
    p, d, _ = _batch(name)
    got = eng.verify_txns_host(p, d)
    assert np.isin(got[1], (0, -1, -2, -3)).all(), np.unique(got[1])        # nothing left in flight (FD_PEND_*)
    ks._check(got, _want(name, sem), (name, what))
    ff, fw = eng.ffull_count(), eng.fwide_count()
    assert fw[0] <= ff[0] and fw[1] <= ff[1], (name, what, ff, fw)
    return got[1], ff, fw


# ---- the fixtures (CPU) ----------------------------------------------------------------------------------------

FRESH = ["one_key", "interleaved", "multi", "edge255", "edge256", "edge257", "bad_sigs", "bad_keys", "torsion",
         "hs_top", "malformed"]
SLOTS, WIDE_SLOTS = 8, 4             # key_cache = 2 and key_wide = 2


def test_fixtures():
    """(CPU only.)  What the GPU cases compare the device's counts with"""
    # the fresh cases fit the 8 slots; some have no more keys than wide slots (every walking wave is wide) and
    # some have more (waves of both kinds)
    nkeys = {name: kf._repeated(name, 4)[0] for name in FRESH}
    assert all(1 <= n <= SLOTS for n in nkeys.values()), nkeys
    assert nkeys["one_key"] == 1 and nkeys["multi"] > WIDE_SLOTS and nkeys["bad_keys"] > WIDE_SLOTS
    assert min(nkeys.values()) <= WIDE_SLOTS < max(nkeys.values())
    assert _walkers("key0_x300") == (1, 300) and _walkers("mixed") == (2, 300)
    # the ends batch: the key's scalar is the one its public key comes from, every signature is valid, and every
    # table meets exactly the ends listed
    assert torsion.encode(torsion._mul(_scalar(0), torsion.BASE)) == ks._key(0)[0]
    picked = _ground()
    assert 24 <= len(picked) <= 72 and _batch("ends")[2] == len(picked) <= 256
    seen = [set() for _ in range(24)]
    for _, k in picked:
        for q, x in enumerate(_wide_digits(k)):
            seen[q].add(x)
            assert -W0 <= x < W0 if q % 3 < 2 else -514 <= x <= 510
    for t in range(8):
        for r in range(3):
            assert set(_ends(t, r)) <= seen[3 * t + r], (t, r)
    assert min(seen[23]) == 0 and max(seen[23]) == 64
    want = _want("ends", 0)
    assert (np.asarray(want[0]) == 0).all() and (np.asarray(want[1]) == 0).all()
    # pins: 20 keys in slots 0..19, the first 16 wide under key_wide = 2 on a context of 32 slots
    assert kp._expect("fifteen", [kp._pub(i) for i in range(20)]) == ((20, 300), 300)
    assert kp._expect("alternate", [kp._pub(i) for i in range(20)]) == ((2, 80), 80)
    assert kp._expect("five", [kp._pub(i) for i in (3, 4, 5)]) == ((3, 5), 5)
    assert _walkers("late") == (4, 40)


# ---- key_full = 2, key_wide = 2, 8 slots: a claim fills its slot at once, the first four wide ---------------------

@_once
def _fresh(name, sem, fold):
    eng = _engine([_batch(name)], sem, fold, key_full=TESTS, key_wide=TESTS, key_cache=TESTS)
    try:
        _, ff, fw = _go(eng, name, sem, "fresh")
        nk = eng.fixed_count()[0]
        assert nk == kf._repeated(name, 4)[0] and ff == (nk, _walkers(name)[1]), (name, ff)
        assert fw[0] == min(nk, WIDE_SLOTS), (name, fw)          # slots 0 .. nk - 1: the first four have wide tables
        if nk <= WIDE_SLOTS:
            assert fw[1] == ff[1], (name, ff, fw)                # every walking wave is of wide keys alone
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("name", FRESH)
def test_fresh_context(name, sem, fold):
    _fresh(name, sem, fold)


# ---- the defaults: claimed, then promoted and wide ---------------------------------------------------------------

@_once
def _three_batches(name, sem, fold):
    eng = _engine([_batch(name)], sem, fold)
    off = _engine([_batch(name)], sem, fold, key_wide=OFF)
    try:
        for run in range(3):
            s, ff, fw = _go(eng, name, sem, run)
            s_off, ff_off, fw_off = _go(off, name, sem, (run, "key_wide=1"))
            np.testing.assert_array_equal(s, s_off)
            assert fw_off == (0, 0) and ff_off == ff
            assert ff == fw == ((0, 0) if run == 0 else _walkers(name)), (name, run, ff, fw)
    finally:
        eng.close()
        off.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("name", ["key0_x300", "mixed"])
def test_three_batches_with_the_defaults(name, sem, fold):
    """Batch 1 claims and walks with doublings; batches 2 and 3 walk 40 additions; with key_wide = 1 they walk 48,
    and the codes are the same"""
    _three_batches(name, sem, fold)


@_once
def _digit_ends(sem, fold):
    eng = _engine([_batch("ends")], sem, fold, key_full=TESTS)
    try:
        s, ff, fw = _go(eng, "ends", sem)
        n = _batch("ends")[2]
        assert (s == 0).all() and ff == fw == (1, n)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_digit_ends(sem, fold):
    """Every wide table read at its identity entry, at its last entry negated and at the last entry a positive digit
    reaches (test_fixtures): every signature verifies"""
    _digit_ends(sem, fold)


@_once
def _shared_wave(sem, fold):
    eng = _engine([_batch("key0_x300"), _batch("mixed")], sem, fold)
    try:
        assert _go(eng, "key0_x300", sem, 1)[1:] == ((0, 0), (0, 0))
        assert _go(eng, "key0_x300", sem, 2)[1:] == ((1, 300), (1, 300))
        s, ff, fw = _go(eng, "mixed", sem, "key 1 is new")
        assert (s == 0).all() and ff == fw == (1, 0)             # key 0 is wide, and no wave is of key 0 alone
        s, ff, fw = _go(eng, "mixed", sem, "key 1 promoted")
        assert (s == 0).all() and ff == fw == (2, 300)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_a_wave_shared_with_a_key_claimed_in_this_batch(sem, fold):
    """... walks with doublings, all of it: its signatures are in neither count"""
    _shared_wave(sem, fold)


# ---- pins ------------------------------------------------------------------------------------------------------

def _pin_engine(batches, sem, fold, **opts):
    o = dict(key_fixed=ON, key_split=0, max_sig=kp.MAX_SIG)
    o.update(opts)
    return _engine(batches, sem, fold, **o)


@_once
def _pins_walk_wide(sem, fold):
    pins = [kp._pub(i) for i in (3, 4, 5)]
    eng = _pin_engine([_batch("five")], sem, fold)
    try:
        eng.set_pinned_keys(pins)
        s, ff, fw = _go(eng, "five", sem, "first batch of the context")
        assert (s == 0).all() and eng.pinned_count() == (3, 5) and ff == fw == (3, 5)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_a_pinned_key_walks_wide_in_the_first_batch(sem, fold):
    _pins_walk_wide(sem, fold)


@_once
def _more_pins_than_wide_slots(sem, fold):
    pins = [kp._pub(i) for i in range(20)]                       # 32 slots, key_wide = 2: slots 0..15 are wide
    eng = _pin_engine([_batch("fifteen"), _batch("alternate"), _batch("late")], sem, fold, key_wide=TESTS)
    try:
        eng.set_pinned_keys(pins)
        s, ff, fw = _go(eng, "alternate", sem, "keys 0 and 1")
        assert (s == 0).all() and ff == fw == (2, 80)
        s, ff, fw = _go(eng, "late", sem, "keys 16..19")
        assert (s == 0).all() and ff == (4, 40) and fw == (0, 0)
        s, ff, fw = _go(eng, "fifteen", sem, "every wave holds all twenty")
        assert (s == 0).all() and ff == (20, 300) and fw == (16, 0)
        # a new set, the other way round: key 19 in slot 0, keys 0..3 in slots 19..16
        eng.set_pinned_keys(pins[::-1])
        s, ff, fw = _go(eng, "alternate", sem, "replaced")
        assert (s == 0).all() and ff == (2, 80) and fw == (0, 0)
        s, ff, fw = _go(eng, "late", sem, "replaced")
        assert (s == 0).all() and ff == fw == (4, 40)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_more_pins_than_wide_slots_and_a_new_set(sem, fold):
    _more_pins_than_wide_slots(sem, fold)


@_once
def _pins_with_the_cache_off(sem, fold):
    pins = [kp._pub(0), kp._pub(1)]
    eng = _pin_engine([_batch("alternate")], sem, fold, key_cache=OFF)
    try:
        eng.set_pinned_keys(pins)
        for run in range(2):
            s, ff, fw = _go(eng, "alternate", sem, run)
            assert (s == 0).all() and ff == fw == (2, 80)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_pins_with_key_cache_off(sem, fold):
    """Every slot is emptied ahead of each batch; the pins get their words back, and their wide tables were built when
    they were pinned"""
    _pins_with_the_cache_off(sem, fold)


@_once
def _pinned_keys_without_tables(sem, fold):
    pins = ks._edge_keys() + [kp._pub(1)]
    eng = _pin_engine([_batch("bad_keys")], sem, fold)
    try:
        kp._check_status(eng.set_pinned_keys(pins), pins)
        first = None
        for run in range(2):
            s, ff, fw = _go(eng, "bad_keys", sem, run)
            keys_sigs, walkers = kp._expect("bad_keys", pins)
            assert ff == fw == (keys_sigs[0], walkers), (ff, fw)  # (a pinned slot counts as full, tables or not)
            first = s if first is None else first
            np.testing.assert_array_equal(first, s)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_pinned_keys_without_tables(sem, fold):
    """An undecodable key, x = 0 with the sign bit and keys of order 4 and 8, pinned beside a good one: nothing is
    built for them, and their signatures replay the status"""
    _pinned_keys_without_tables(sem, fold)


# ---- 8 slots: pmax = 2 ---------------------------------------------------------------------------------------------

@_once
def _promotion_cap(cache, max_sig, wide, sem, fold):
    eng = _engine([_batch("eight_a")], sem, fold, max_sig=max_sig, key_cache=cache, key_wide=wide)
    wcap = 4 if wide == TESTS else 8
    try:
        for run in range(6):
            s, ff, fw = _go(eng, "eight_a", sem, run)
            assert (s == 0).all()
            if cache == ON:
                assert ff == (min(8, 2 * run), 32 if run >= 4 else 0), (run, ff)     # (the 32 signatures are one wave)
                assert min(8, 2 * run) - (8 - wcap) <= fw[0] <= min(wcap, 2 * run), (run, fw)
                assert fw[1] == (32 if run >= 4 and wcap == 8 else 0), (run, fw)
            else:
                assert ff[0] <= min(8, 2 * run) and fw[0] <= wcap and fw[1] in (0, 32)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("wide", [ON, TESTS])
@pytest.mark.parametrize("how,cache,max_sig", kfull.EIGHT)
def test_promotions_reach_the_wide_state_slot_by_slot(how, cache, max_sig, wide, sem, fold):
    """8 keys resident in 8 slots, two promoted per batch; a promoted slot below wcap is wide in the same batch"""
    _promotion_cap(cache, max_sig, wide, sem, fold)


# ---- the latency path -------------------------------------------------------------------------------------------

@_once
def _latency(sem):
    eng = _engine([_batch("key0_x300")], sem, key_full=TESTS, small_batch_max=-1)
    try:
        for run in range(2):
            s, ff, fw = _go(eng, "key0_x300", sem, ("latency", run))
            assert (s == 0).all() and ff == fw == (0, 0) and eng.fixed_count() == (0, 0)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_the_latency_path_ignores_it(sem):
    _latency(sem)
