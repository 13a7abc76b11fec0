"""GPU: the half-size throughput path decodes each distinct public key of a batch once
(fd_keydedup_kernel; DESIGN "One decode per distinct key").

Every case runs on small batches forced onto the throughput path (small_batch_max = 0), in both
result-code semantics, with the de-duplication on (the default), off (fdgpu_debug_opts_t.key_dedup = 1:
the kernels without it) and, where named, with the tests' 64-slot table and two probes (key_dedup = 2: most
keys find no slot and fall back to being their own representative).  The transaction and per-signature
codes equal the CPU oracle's in every mode, so on and off are equal too.  Which signature of a key
becomes its representative differs from run to run and must not show.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS = 16
ON, OFF, TINY = 0, 1, 2


@pytest.fixture(scope="module")
def fa():
    import firedancer_amd
    firedancer_amd.load_library()
    return firedancer_amd


def _engine(fa, n_txn, nsig, nbytes, sem, mode, force_slow=0):
    from firedancer_amd import engine
    engine.debug_set_opts(half=1, small_batch_max=0, half_force_slow=force_slow, key_dedup=mode)
    try:
        return fa.Engine(device=0, max_txn=n_txn, max_sig=nsig, max_payload=nbytes, semantics=sem)
    finally:
        engine.debug_reset_opts()


def _run(fa, batch, sem, mode, force_slow=0):
    payload, desc, nsig = batch
    eng = _engine(fa, len(desc), nsig, payload.nbytes, sem, mode, force_slow)
    try:
        t, s = eng.verify_txns_host(payload, desc)
        return t, s, eng.slow_count(), eng.key_count()
    finally:
        eng.close()


def _edge_keys():
    """From the golden edge encodings: a key that does not decode, two small-order keys (orders 4 and 8)
    and y = 1 with the sign bit set (x = 0: rejected at the decode by the AVX-512 semantics only)."""
    from oracle.oracle import Oracle
    from tests.golden_io import load_vectors
    v = load_vectors()
    e = v["set_id"] == 4
    encs = sorted({bytes(x) for x in v["pub"][e]} | {bytes(x[:32]) for x in v["sig"][e]})
    o = Oracle()
    undec = next(x for x in encs if o.point_decode(x, 1)[0] == 1)
    x0sign = next(x for x in encs if o.point_decode(x, 0)[0] == 2)
    small4 = bytes(32)
    small8 = bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05")
    assert small4 in encs and small8 in encs
    return [undec, x0sign, small4, small8]


def _key_at(payload, desc, t, j=0):
    at = int(desc["payload_off"][t]) + int(desc["acct_addr_off"][t]) + 32 * j
    return payload[at: at + 32]


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(payload, desc, nsig) of a named case, built once."""
    from firedancer_amd import synth
    mk = synth.make_batch
    if name == "one_key":            # every signature by one key
        p, d, _, n = mk(3000, synth.SMALL_MSG, 1, 0.1, seed=11, nkeys=1, threads=THREADS)
    elif name == "all_distinct":     # signer (7 t + r) mod nkeys, r < 4: no two transactions share a key
        p, d, _, n = mk(3000, synth.SMALL_MSG, 1, 0.1, seed=12, nkeys=7 * 3000 + 4, threads=THREADS)
        keys = {_key_at(p, d, t).tobytes() for t in range(0, 3000, 3)}
        assert len(keys) >= 950          # (the injected faults put a few bad keys in, shared)
    elif name == "default_keys":
        p, d, _, n = mk(3000, synth.SMALL_MSG, 1, 0.1, seed=13, threads=THREADS)
    elif name.startswith("size_"):   # the block and wave edges of the compaction
        p, d, _, n = mk(int(name[5:]), synth.SMALL_MSG, 1, 0.1, seed=14 + int(name[5:]), nkeys=5, threads=THREADS)
    elif name == "multi":            # 1-12 signers of 8 keys: one key at several indices of a transaction
        p, d, _, n = mk(1000, synth.MULTI, 12, 0.1, seed=15, nkeys=8, threads=THREADS)
        t = int(np.argmax(d["sig_cnt"]))
        ks = [_key_at(p, d, t, j).tobytes() for j in range(int(d["sig_cnt"][t]))]
        assert len(ks) == 12 and len(set(ks)) < 12
    elif name == "bad_keys":         # configs[2]'s recipe, and four bad keys each shared by ~100 signatures
        p, d, _, n = mk(2000, synth.LARGE_NOOP, 1, 0.1, seed=16, nkeys=8, threads=THREADS)
        for k, enc in enumerate(_edge_keys()):
            for t in range(3 + k, 2000, 20):
                _key_at(p, d, t)[:] = np.frombuffer(enc, np.uint8)
    elif name == "one_byte":         # copies of one key with one bit flipped in its first, middle, last byte
        p, d, _, n = mk(400, synth.SMALL_MSG, 1, 0.0, seed=17, nkeys=1, threads=THREADS)
        for t in range(400):
            if t % 4:
                _key_at(p, d, t)[(0, 0, 15, 31)[t % 4]] ^= (1, 1, 0x10, 0x40)[t % 4]
    elif name == "malformed":        # transactions that fail the bounds check among duplicates of their key
        p, d, _, n = mk(600, synth.SMALL_MSG, 1, 0.1, seed=18, nkeys=3, threads=THREADS)
        for t in range(2, 600, 5):
            d["payload_sz"][t] = (int(d["acct_addr_off"][t]) + 31, int(d["message_off"][t]) - 1)[t & 1]
    else:
        raise KeyError(name)
    return p, d, n


@functools.lru_cache(maxsize=None)
def _want(name, sem):
    from oracle.oracle import Oracle
    p, d, n = _batch(name)
    return Oracle().verify_txns(p, d, n, sem=sem, threads=THREADS)


@functools.lru_cache(maxsize=None)
def _distinct(name, slots=None):
    """Decodes the batch needs: its distinct keys among well-formed transactions, and one per signature of
    a malformed one (the oracle's bounds check, fd_ed25519_oracle.c txn_bounds_ok).  With slots: the
    fewest decodes when only that many keys can be shared (the most frequent ones, at best)."""
    import collections
    p, d, n = _batch(name)
    keys, lone = collections.Counter(), 0
    for t in range(len(d)):
        c, sz = int(d["sig_cnt"][t]), int(d["payload_sz"][t])
        if (int(d["signature_off"][t]) + 64 * c > sz or int(d["acct_addr_off"][t]) + 32 * c > sz
                or int(d["message_off"][t]) > sz):
            lone += c
        else:
            keys.update(_key_at(p, d, t, j).tobytes() for j in range(c))
    if slots is None:
        return len(keys) + lone
    top = keys.most_common(slots)
    return lone + sum(keys.values()) - sum(c for _, c in top) + len(top)


def _check(got, want, what):
    for g, w, kind in ((got[0], want[0], "txn"), (got[1], want[1], "sig")):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, kind, [(int(i), int(g[i]), int(w[i])) for i in bad[:16]])


CASES = ["one_key", "all_distinct", "default_keys", "size_1", "size_255", "size_256", "size_257", "size_3001",
         "multi", "bad_keys", "one_byte", "malformed"]


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_codes_equal_oracle_on_and_off(fa, name, sem):
    want = _want(name, sem)
    on = _run(fa, _batch(name), sem, ON)
    off = _run(fa, _batch(name), sem, OFF)
    _check(on, want, "on")
    _check(off, want, "off")
    np.testing.assert_array_equal(on[1], off[1])
    # no silent fallback: every distinct key is decoded at least once, and with the table at a load of at
    # most 0.5 a run of 16 taken slots (a key decoded a second time) is rarer than one key in 10^4
    k = _distinct(name)
    assert k <= on[3] <= k + k // 50 + 1, (on[3], k)
    assert off[3] == 0


def test_cases_have_teeth():
    """The fixtures hold what they are named for (CPU only, but they are this module's)."""
    _, s = _want("one_byte", 0)
    assert (s[0::4] == 0).all() and (s[np.arange(400) % 4 != 0] != 0).all()     # a shared representative would pass them
    p, d, n = _batch("bad_keys")
    for sem in (0, 1):
        _, s = _want("bad_keys", sem)
        for k in range(4):
            assert (s[3 + k: 2000: 20] != 0).all()
    _, s = _want("malformed", 0)
    assert (s[2::5] == -1).all() and (s == 0).sum() > 300
    _, s = _want("one_key", 0)
    assert (s == 0).sum() > 2500 and (s != 0).sum() > 100


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", ["one_key", "multi", "bad_keys"])
def test_forced_slow_list_with_shared_keys(fa, name, sem):
    """Every third signature takes the full walk off the slow list, whose -A gathers go through the
    representative's table.  FD_PSTAT_SLOW is the signature's own: a representative on the list must not
    take its key's other signatures out of the half-size walk (their code would stay in flight), nor the
    other way round."""
    want = _want(name, sem)
    nsig = _batch(name)[2]
    for mode in (ON, OFF):
        t, s, slow, _ = _run(fa, _batch(name), sem, mode, force_slow=3)
        assert 0 < slow <= (nsig + 2) // 3
        assert np.isin(s, (0, -1, -2, -3)).all(), np.unique(s)          # nothing left in flight (FD_PEND_*)
        assert (s[want[1] == 0] == 0).all()                             # no valid signature rejected
        _check((t, s), want, mode)


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", ["all_distinct", "default_keys", "multi", "bad_keys"])
def test_tiny_table_falls_back_to_own_representative(fa, name, sem):
    """64 slots and two probes for up to ~6,500 signatures: a lane that finds neither its key nor a free
    slot decodes its key itself.  Same codes."""
    got = _run(fa, _batch(name), sem, TINY)
    _check(got, _want(name, sem), "tiny")
    k, nsig = _distinct(name), _batch(name)[2]
    # 64 slots: at most 64 keys are shared, the signatures of every other key decode it themselves
    assert max(k, _distinct(name, 64)) <= got[3] <= nsig, (got[3], k, _distinct(name, 64))
    _check(_run(fa, _batch(name), sem, TINY, force_slow=3), _want(name, sem), "tiny+slow")


@pytest.mark.parametrize("mode", [ON, TINY])
def test_context_reuse_with_other_keys_at_the_same_indices(fa, mode):
    """Two batches back to back on one context, then the first again: the second has other keys (and bad
    keys) at the same signature indices, so a table slot or a representative left from the batch before
    would give a wrong point."""
    a, b = _batch("default_keys"), _batch("size_3001")
    c = _batch("bad_keys")
    eng = _engine(fa, 3001, 3001, max(x[0].nbytes for x in (a, b, c, _batch("all_distinct"))), 0, mode)
    try:
        # After a batch in which more than 7/8 of the signatures were representatives, the next one on the
        # context is de-duplicated only in its first workgroups (the sample: 1 of these batches' 12), and
        # the sample's own share decides for the batch after it ("B" below; "N": in full).
        d, one = _batch("all_distinct"), _batch("one_key")
        seq = (("default_keys", a, "N"), ("size_3001", b, "N"), ("bad_keys", c, "N"), ("default_keys", a, "N"),
               ("one_key", one, "N"), ("all_distinct", d, "N"), ("all_distinct", d, "B"), ("one_key", one, "B"),
               ("default_keys", a, "N"), ("all_distinct", d, "N"))
        for name, batch, how in seq:
            got = eng.verify_txns_host(batch[0], batch[1])
            _check(got, _want(name, 0), name)
            if mode == ON:
                k, nsig, cnt = _distinct(name), batch[2], eng.key_count()
                if how == "N":
                    assert k <= cnt <= k + k // 50 + 1, (name, cnt, k)
                else:
                    assert max(k, nsig - 256) <= cnt <= nsig, (name, cnt, k)
    finally:
        eng.close()
