"""GPU: the signatures of a public key a batch repeats walk 64 doublings instead of 128
(fd_keysplit_kernel, fd_lat_skew, the hot body of fd_dsmh_kernel).

Every case runs on small batches forced onto the throughput path (small_batch_max = 0), in both result-code
semantics, with fdgpu_debug_opts_t.key_split 0 (on: a key is hot from 8 signatures), 1 (off: the kernels and
launches without it) and 2 (tests: hot from 2 signatures), and with the split on also through the carry-folded
kernels the large batches use (nofold_max = 0).  The transaction and per-signature codes equal the CPU
oracle's in every mode, so the modes are equal to each other too, and the device's count of hot keys and hot
signatures is the batch's own, so the split cannot be silently off.
"""
import collections
import functools
import hashlib
import os

import numpy as np
import pytest

from tests import torsion

pytestmark = pytest.mark.gpu

THREADS = 16
ON, OFF, TWO = 0, 1, 2
HOT_MIN = {ON: 8, TWO: 2}
HERE = os.path.dirname(os.path.abspath(__file__))
L = torsion.L


@pytest.fixture(scope="module")
def fa():
    import firedancer_amd
    firedancer_amd.load_library()
    return firedancer_amd


def _engine(fa, n_txn, nsig, nbytes, sem, mode, force_slow=0, fold=False):
    from firedancer_amd import engine
    engine.debug_set_opts(half=1, small_batch_max=0, half_force_slow=force_slow, key_split=mode,
                          nofold_max=0 if fold else -1)
    try:
        return fa.Engine(device=0, max_txn=n_txn, max_sig=nsig, max_payload=nbytes, semantics=sem)
    finally:
        engine.debug_reset_opts()


@functools.lru_cache(maxsize=None)
def _run(name, sem, mode, force_slow=0, fold=False):
    """(txn codes, signature codes, slow count, (hot keys, hot signatures)) of one batch on a context of its
    own.  Run once: this module chooses its engine options itself, so the suite's engine-path parameter
    (tests/conftest.py) only repeats the assertions on these results."""
    import firedancer_amd as fa
    fa.load_library()
    payload, desc, nsig = _batch(name)
    eng = _engine(fa, len(desc), nsig, payload.nbytes, sem, mode, force_slow, fold)
    try:
        t, s = eng.verify_txns_host(payload, desc)
        return t, s, eng.slow_count(), eng.hot_count()
    finally:
        eng.close()


# ---- batches -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def _key(i):
    prv = hashlib.sha256(b"key_split %d" % i).digest()
    return _oracle().public_from_private(prv), prv


def _sign(i, msg):
    pub, prv = _key(i)
    return _oracle().sign(msg, pub, prv), pub


def _msg(t, n=48):
    return hashlib.sha512(b"msg %d" % t).digest()[:n] * 2


def _pack(txns):
    """(payload, desc, nsig) from [(msg, [(sig64, pub32), ...])]: signatures, keys, message."""
    from firedancer_amd.engine import DESC_DTYPE
    desc = np.zeros(len(txns), DESC_DTYPE)
    parts, pos, nsig = [], 0, 0
    for t, (msg, signers) in enumerate(txns):
        c = len(signers)
        body = b"".join(s for s, _ in signers) + b"".join(p for _, p in signers) + msg
        desc[t] = (pos, nsig, len(body), 96 * c, 64 * c, 0, c)
        body += bytes(-len(body) % 16)
        parts.append(body)
        pos += len(body)
        nsig += c
    payload = np.frombuffer(b"".join(parts) + bytes(1024), np.uint8).copy()
    return payload, desc, nsig


def _single(keys):
    """One single-signer transaction per entry of keys (key numbers), valid."""
    return [(_msg(t), [_sign(k, _msg(t))]) for t, k in enumerate(keys)]


def _edge_keys():
    """From the golden edge encodings: a key that does not decode, y = 1 with the sign bit set (x = 0: rejected
    at the decode by the AVX-512 semantics only) and two small-order keys (orders 4 and 8)."""
    from tests.golden_io import load_vectors
    v = load_vectors()
    e = v["set_id"] == 4
    encs = sorted({bytes(x) for x in v["pub"][e]} | {bytes(x[:32]) for x in v["sig"][e]})
    o = _oracle()
    undec = next(x for x in encs if o.point_decode(x, 1)[0] == 1)
    x0sign = next(x for x in encs if o.point_decode(x, 0)[0] == 2)
    small4 = bytes(32)
    small8 = bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05")
    assert small4 in encs and small8 in encs
    return [undec, x0sign, small4, small8]


def _torsion_txns(per_kind=10):
    """tests/torsion.py's four kinds with one public key per kind, repeated: A = [a]B + T for the three kinds
    with a torsion-carrying A, a clean A under torsion-carrying R for the fourth."""
    import random
    rng = random.Random(20261019)
    t8 = torsion.torsion8(rng)
    txns, codes = [], []
    for kind in ("A_mixed", "R_mixed", "both_cancel", "both_mixed"):
        a = rng.randrange(1, L)
        ti = rng.randrange(1, 8) if kind != "R_mixed" else 0
        A = torsion._add(torsion._mul(a, torsion.BASE), t8[ti])
        a_enc = torsion.encode(A)
        made = 0
        while made < per_kind:
            r = rng.randrange(1, L)
            msg = rng.randbytes(rng.randrange(1, 120))
            rb = torsion._mul(r, torsion.BASE)
            if kind == "both_cancel":
                hit = None
                for tj in range(1, 8):
                    r_enc = torsion.encode(torsion._add(rb, t8[tj]))
                    k = torsion._k(r_enc, a_enc, msg)
                    if torsion._eq(torsion._add(t8[tj], torsion._mul(k, t8[ti])), torsion.IDENT):
                        hit = (r_enc, k)
                        break
                if hit is None:
                    continue
                r_enc, k = hit
            else:
                tj = rng.randrange(1, 8) if kind in ("R_mixed", "both_mixed") else 0
                r_enc = torsion.encode(torsion._add(rb, t8[tj]))
                k = torsion._k(r_enc, a_enc, msg)
            s = (r + k * a) % L
            lhs = torsion._add(torsion._mul(s, torsion.BASE), torsion._neg(torsion._mul(k, A)))
            codes.append(0 if torsion._eq(lhs, torsion._point_from_enc(r_enc)) else -3)
            txns.append((msg, [(r_enc + s.to_bytes(32, "little"), a_enc)]))
            made += 1
    return txns, codes


def _hs_top_txns(reps=9):
    """The transactions of tests/golden/hs_top.npz (valid; both half-size scalars below 2^120), each reps times."""
    hs = dict(np.load(os.path.join(HERE, "golden", "hs_top.npz")))
    txns = []
    for i in range(len(hs["txn"])):
        t = hs["txn"][i].tobytes()[: int(hs["payload_sz"][i])]
        so, ao, mo = int(hs["signature_off"][i]), int(hs["acct_addr_off"][i]), int(hs["message_off"][i])
        txns += [(t[mo:], [(t[so:so + 64], t[ao:ao + 32])])] * reps
    return txns


COUNTS = (1, 2, 3, 7, 8, 9)          # FD_HOT_MIN - 1, FD_HOT_MIN, FD_HOT_MIN + 1 for both values of it


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(payload, desc, nsig) of a named case, built once."""
    if name == "two_keys":           # 2 keys x 300 signatures: the hot list crosses wave and block edges
        txns = _single([t & 1 for t in range(600)])
    elif name == "interleaved":      # three hot keys among keys seen once: every source wave holds both
        txns = _single([(t % 3) if t % 2 else 1000 + t for t in range(400)])
    elif name == "counts":           # keys with exactly 1, 2, 3, 7, 8, 9 signatures, shuffled
        ks = [10 + i for i, c in enumerate(COUNTS) for _ in range(c)]
        np.random.default_rng(5).shuffle(ks)
        txns = _single(ks)
    elif name == "no_hot":           # every key once
        txns = _single(range(2000, 2300))
    elif name == "no_cold":          # three keys, 100 signatures each
        txns = _single([t % 3 for t in range(300)])
    elif name == "multi":            # two signers per transaction, one hot and one cold, in either order
        txns = []
        for t in range(150):
            m = _msg(t, 64)
            pair = [_sign(t % 2, m), _sign(3000 + t, m)]
            txns.append((m, pair if t % 3 else pair[::-1]))
    elif name == "bad_sigs":         # a hot key with a bad S, a wrong message and a corrupted R among valid ones
        txns = []
        for t in range(120):
            m = _msg(t)
            sig, pub = _sign(7, m)
            sig = bytearray(sig)
            if t % 8 == 1:
                sig[40] ^= 1                                     # S changed, still below l
            elif t % 8 == 3:
                sig[32:] = (L + t).to_bytes(32, "little")        # S >= l
            elif t % 8 == 5:
                m = m[:-1] + bytes([m[-1] ^ 0x80])               # another message
            elif t % 8 == 7:
                sig[3] ^= 0x10                                   # R corrupted
            txns.append((m, [(bytes(sig), pub)]))
    elif name == "bad_keys":         # an undecodable, an x = 0 with sign and two small-order keys, 12 signatures each
        txns = []
        for t in range(96):
            m = _msg(t)
            if t % 2:
                txns.append((m, [(_sign(1, m)[0], _edge_keys()[(t // 2) % 4])]))
            else:
                txns.append((m, [_sign(1, m)]))
    elif name == "torsion":
        txns = _torsion_txns()[0]
    elif name == "malformed":        # transactions that fail the bounds check among hot signatures
        p, d, n = _pack(_single([t % 2 for t in range(300)]))
        d = d.copy()
        for t in range(2, 300, 5):
            d["payload_sz"][t] = (int(d["acct_addr_off"][t]) + 31, int(d["message_off"][t]) - 1)[t & 1]
        return p, d, n
    elif name == "hs_top":
        txns = _hs_top_txns()
    else:
        raise KeyError(name)
    return _pack(txns)


@functools.lru_cache(maxsize=None)
def _want(name, sem):
    p, d, n = _batch(name)
    return _oracle().verify_txns(p, d, n, sem=sem, threads=THREADS)


@functools.lru_cache(maxsize=None)
def _hot(name, hot_min):
    """(hot keys, hot signatures) the batch holds: keys of well-formed transactions with >= hot_min signatures."""
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
    hot = [c for c in keys.values() if c >= hot_min]
    return len(hot), sum(hot)


def _check(got, want, what):
    for g, w, kind in ((got[0], want[0], "txn"), (got[1], want[1], "sig")):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, kind, [(int(i), int(g[i]), int(w[i])) for i in bad[:16]])


CASES = ["two_keys", "interleaved", "counts", "no_hot", "no_cold", "multi", "bad_sigs", "bad_keys", "torsion",
         "malformed", "hs_top"]
MODES = [(ON, False), (ON, True), (OFF, False), (TWO, False)]


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_codes_equal_oracle_in_every_mode(fa, name, sem):
    want = _want(name, sem)
    sigs = []
    for mode, fold in MODES:
        got = _run(name, sem, mode, fold=fold)
        _check(got, want, (mode, fold))
        sigs.append(got[1])
        assert got[3] == ((0, 0) if mode == OFF else _hot(name, HOT_MIN[mode])), (mode, fold, got[3])
    for s in sigs[1:]:
        np.testing.assert_array_equal(sigs[0], s)


def test_cases_have_teeth():
    """The fixtures hold what they are named for (CPU only, but they are this module's)."""
    assert _hot("counts", 8) == (2, 17) and _hot("counts", 2) == (5, 29)
    assert _hot("no_hot", 2) == (0, 0) and _hot("no_cold", 8) == (3, 300)
    assert _hot("two_keys", 8) == (2, 600) and _hot("interleaved", 8) == (3, 200)
    assert _hot("multi", 8) == (2, 150) and _hot("hs_top", 8)[1] == _batch("hs_top")[2]
    for sem in (0, 1):
        _, s = _want("bad_sigs", sem)
        t = np.arange(120)
        assert (s[t % 2 == 0] == 0).all() and (s[t % 8 == 3] == -1).all()
        assert (s[(t % 8 == 1) | (t % 8 == 5)] == -3).all() and (s[t % 8 == 7] != 0).all()
        _, s = _want("bad_keys", sem)
        assert (s[0::2] == 0).all() and (s[1::2] != 0).all()
        _, s = _want("hs_top", sem)
        assert (s == 0).all()
        _, s = _want("torsion", sem)
        codes = np.array(_torsion_txns()[1], np.int8)
        np.testing.assert_array_equal(s, codes)
        # R's torsion alone never cancels, the cancelling kind always; the other two cancel by chance (k T = -T')
        assert (codes[10:20] == -3).all() and (codes[20:30] == 0).all() and (codes != 0).sum() >= 25
    _, s = _want("malformed", 0)
    assert (s[2::5] == -1).all() and (s == 0).sum() > 200
    _, s = _want("multi", 0)
    assert (s == 0).all()


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", ["two_keys", "multi", "torsion", "bad_keys"])
def test_forced_slow_list_with_hot_signatures(fa, name, sem):
    """Every third signature takes the full walk off the slow list: a hot one's digits lie at its place in the
    hot order, its -A table at its representative."""
    want = _want(name, sem)
    nsig = _batch(name)[2]
    for mode, fold in MODES:
        t, s, slow, _ = _run(name, sem, mode, force_slow=3, fold=fold)
        assert 0 < slow <= (nsig + 2) // 3
        assert np.isin(s, (0, -1, -2, -3)).all(), np.unique(s)          # nothing left in flight (FD_PEND_*)
        _check((t, s), want, (mode, fold))


@pytest.mark.parametrize("mode", [ON, TWO])
def test_one_context_hot_cold_and_bypass_batches(fa, mode):
    """One context, batches of repeated keys, of distinct keys and -- after a batch of distinct keys -- batches
    that are only sampled by the de-duplication (which counts nothing, so they hold no hot key): counters,
    the order and the high tables of the batch before must not show."""
    names = ("no_cold", "no_hot", "counts", "two_keys", "bad_keys")
    b = {n: _batch(n) for n in names}
    eng = _engine(fa, 600, 600, max(x[0].nbytes for x in b.values()), 0, mode)
    try:
        # "B": sampled only, because more than 7/8 of the signatures of the batch before were representatives
        seq = (("no_cold", "N"), ("two_keys", "N"), ("no_hot", "N"), ("no_cold", "B"), ("no_cold", "N"),
               ("counts", "N"), ("no_hot", "N"), ("no_hot", "B"), ("two_keys", "B"), ("bad_keys", "N"),
               ("no_cold", "N"))
        for name, how in seq:
            got = eng.verify_txns_host(b[name][0], b[name][1])
            _check(got, _want(name, 0), (name, how))
            assert eng.hot_count() == ((0, 0) if how == "B" else _hot(name, HOT_MIN[mode])), (name, how)
    finally:
        eng.close()
