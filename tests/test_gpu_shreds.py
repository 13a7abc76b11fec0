"""GPU: Merkle shreds verified from descriptors (fdgpu_ed25519_verify_shreds_device / _host, DESIGN 22:
fd_shred_slot_kernel, fd_shred_root_kernel and fd_shred_flag_kernel around an unchanged batch) and the batch SHA-256
beside them (fd_sha256_batch_kernel).

Expected values never come from the code under test: the fixture's are the reference's own recorded results
(tests/golden/shreds.npz: fd_shred_parse, fd_shred_merkle_root and fd_ed25519_verify in both semantics); the built
shreds' are tests/shred_model.py's, which tests/test_shred_desc.py holds against that fixture, and the CPU oracle's
verify; the hashes' are hashlib's.

test_fixture_parity_on_every_engine_path runs under the suite's engine-path parameter (tests/conftest.py).  The other
scenarios choose their options themselves, so they run on the GPU once (_once) and the suite's repeats only find
that they passed.
"""
import functools
import hashlib

import numpy as np
import pytest

from firedancer_amd import engine
from tests import shred_model as sm
from tests import test_gpu_key_split as ks
from tests.test_gpu_sigs import _Arena, _once, _refused
from tests.test_shred_desc import case_bytes, expected, fixture

pytestmark = pytest.mark.gpu

DESC, PARSE, MERKLE = engine.FDGPU_ERR_DESC, engine.FDGPU_ERR_SHRED_PARSE, engine.FDGPU_ERR_SHRED_MERKLE
NO_SIG, STRICT = engine.FDGPU_SHRED_NO_SIG, engine.FDGPU_SHRED_STRICT_LEAF
COUNTS = (1, 63, 64, 65, 255, 256, 257)
KINDS = sm.DATA_TYPES + sm.CODE_TYPES


def _engine(n, payload=0, shreds=None, keys=8, defaults=True, semantics=0, **opts):
    import firedancer_amd as fa
    fa.load_library()
    if defaults:
        engine.debug_reset_opts()
    if opts:
        engine.debug_set_opts(**opts)
    try:
        eng = fa.Engine(device=0, max_txn=n, max_sig=n, max_payload=payload, semantics=semantics)
    finally:
        if opts:
            engine.debug_reset_opts()
    if shreds:
        eng.shreds_prepare(shreds, keys)
    return eng


def _number(desc):
    """the descriptors with sig_idx numbering the records that name a key, and their count"""
    d = desc.copy()
    keyed = d["key_idx"] != NO_SIG
    d["sig_idx"][keyed] = np.arange(int(keyed.sum()))
    return d, int(keyed.sum())


def _device(eng, arena, arena_sz, desc, sig_cnt, keys, want_root=True):
    import torch
    a = torch.from_numpy(arena).cuda()
    d = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).cuda()
    k = torch.from_numpy(np.ascontiguousarray(keys, np.uint8).reshape(-1).copy()).cuda() if len(keys) else None
    out = torch.full((len(desc),), 7, dtype=torch.int8, device="cuda")
    root = torch.full((len(desc), 32), 0x5A, dtype=torch.uint8, device="cuda") if want_root else None
    eng.verify_shreds_device(a.data_ptr(), arena_sz, d.data_ptr(), len(desc), sig_cnt, k.data_ptr() if k is not None else None,
                             len(keys), out.data_ptr(), root.data_ptr() if want_root else None,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (root.cpu().numpy() if want_root else None)


def _registered(eng, arena, arena_sz, desc, keys, want_root=True):
    engine.host_register(arena)
    try:
        return eng.verify_shreds_host(arena, desc, np.ascontiguousarray(keys, np.uint8), arena_sz, want_root)
    finally:
        engine.host_unregister(arena)


def _plain(eng, arena, arena_sz, desc, keys, want_root=True):
    return eng.verify_shreds_host(arena.copy(), desc, np.ascontiguousarray(keys, np.uint8), arena_sz, want_root)


def _all_forms(eng, arena, arena_sz, desc, keys, want, want_root, what):
    d, nsig = _number(desc)
    forms = (("device", lambda: _device(eng, arena, arena_sz, d, nsig, keys)),
             ("registered", lambda: _registered(eng, arena, arena_sz, desc, keys)),
             ("plain", lambda: _plain(eng, arena, arena_sz, desc, keys)))
    for name, f in forms:
        got, root = f()
        np.testing.assert_array_equal(got, want, err_msg=str((what, name, "codes")))
        np.testing.assert_array_equal(root, want_root, err_msg=str((what, name, "roots")))


def _place(shreds, szs=None, seed=1, last_flush=False):
    """An arena holding the shreds, number i at offset i mod 8 (mod 16: every alignment of a dword and a quad) behind
    a gap of junk, and their descriptors (no key).  last_flush: the last shred ends at the arena's last byte."""
    ar = _Arena(seed)
    desc = np.zeros(len(shreds), engine.SHRED_DESC_DTYPE)
    for i, s in enumerate(shreds):
        desc[i]["off"] = ar.put(s, (5 * i + i // 16) % 16)
        desc[i]["sz"] = len(s) if szs is None else szs[i]
    desc["key_idx"] = NO_SIG
    if not last_flush:
        ar.put(bytes(16))
    arena, n = ar.array()
    return arena, n, desc


# ---- 1: the reference's fixture on every engine path ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fixture_batch():
    g = fixture()
    n = len(g["c_base"])
    shreds = [case_bytes(g, i) for i in range(n)]
    arena, arena_sz, desc = _place(shreds, [int(z) for z in g["c_sz"]], seed=11)
    desc["key_idx"] = g["c_key"]
    want = {}
    for sem in (0, 1):
        ex = [expected(g, i, sem) for i in range(n)]
        want[sem] = (np.array([c for c, _ in ex], np.int8), np.frombuffer(b"".join(r for _, r in ex), np.uint8).reshape(n, 32))
    return arena, arena_sz, desc, g["keys"], want


def test_fixture_parity_on_every_engine_path(engine_path):
    """The 186 shreds of the reference's archives and their mutants, each with a signature slot of its own: codes and
    roots equal the reference's in both semantics, through the device form and both host branches"""
    arena, arena_sz, desc, keys, want = _fixture_batch()
    n = len(desc)
    assert (want[0][0][:186] == 0).all() and {0, -1, -2, -3, PARSE, MERKLE} <= set(want[0][0].tolist())
    assert (want[0][0] != want[1][0]).any()
    for sem in (engine.SEMANTICS_AVX512, engine.SEMANTICS_REF):
        eng = _engine(n, payload=n * 1232, shreds=n, keys=len(keys), defaults=False, semantics=sem)
        try:
            _all_forms(eng, arena, arena_sz, desc, keys, want[sem][0], want[sem][1], (engine_path, sem))
        finally:
            eng.close()


# ---- 2: built shreds ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _built_batch():
    """Valid shreds of every kind and depth at the leaf indices around 2^depth, with and without STRICT_LEAF, leaf 511
    and 512, and a few with a broken signature; the last one ends the arena"""
    o = ks._oracle()
    specs = []
    for kind in KINDS:
        for d in range(10):
            for leaf in sorted({0, (1 << d) - 1, 1 << d}):
                if kind in sm.CODE_TYPES and not 1 <= leaf <= 255:
                    continue
                specs.append((kind, d, leaf))
    specs += [(0x80, 9, 511), (0x90, 4, 511), (0x80, 9, 512), (0xb0, 3, 512)]
    shreds, pubs = [], []
    for t, (kind, d, leaf) in enumerate(specs):
        if leaf > 511:                                            # the builder makes valid shreds only: idx moved after it
            s = bytearray(sm.build(kind, d, 511, t, lambda r: ks._sign(t % 4, r)[0]))
            s[0x49:0x4d] = (int.from_bytes(s[0x4f:0x53], "little") + leaf).to_bytes(4, "little")
        else:
            s = bytearray(sm.build(kind, d, leaf, t, lambda r: ks._sign(t % 4, r)[0]))
        if t % 7 == 3:
            s[33 + t % 30] ^= 0x04                                 # S
        if t % 11 == 5:
            s[100 + t] ^= 0x80                                     # the leaf
        shreds.append(bytes(s))
    shreds.append(sm.build(0x90, 6, 63, 999, lambda r: ks._sign(1, r)[0]))
    arena, arena_sz, d1 = _place(shreds, seed=12, last_flush=True)
    assert int(d1["off"][-1]) + int(d1["sz"][-1]) == arena_sz and set((d1["off"] % 8).tolist()) == set(range(8))
    keys = np.frombuffer(b"".join(ks._key(i)[0] for i in range(4)), np.uint8).reshape(4, 32)
    d1["key_idx"] = [t % 4 for t in range(len(shreds) - 1)] + [1]
    d2 = d1.copy()
    d2["flags"] = STRICT
    desc = np.concatenate([d1, d2])
    codes, roots = [], []
    for flags, dd in ((0, d1), (STRICT, d2)):
        for t, s in enumerate(shreds):
            code, root = sm.outcome(s, len(s), flags)
            if not code:
                code = o.verify(root, s[:64], keys[dd[t]["key_idx"]].tobytes(), 0)
            codes.append(code)
            roots.append(root if root is not None else bytes(32))
    want = np.array(codes, np.int8)
    want_root = np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32)
    return arena, arena_sz, desc, keys, want, want_root, len(shreds)


@_once
def _built():
    arena, arena_sz, desc, keys, want, want_root, m = _built_batch()
    # without the flag only a leaf past 511 is refused: leaf 2^9 of the three data kinds and the two leaf-512 shreds
    assert (want[:m] == 0).sum() > 100 and (want[:m] == MERKLE).sum() == 5 and (want[:m] < 0).sum() > 20
    assert (want[m:] == MERKLE).sum() > 30 and want[m - 1] == 0 and want[-1] == 0
    n = len(desc)
    eng = _engine(n, payload=n * 1232, shreds=n, keys=4)
    try:
        _all_forms(eng, arena, arena_sz, desc, keys, want, want_root, "all")
        for cnt in COUNTS:
            # the last record, whose shred ends the arena, closes every count
            idx = np.concatenate([np.arange(cnt - 1), [m - 1]])
            d, nsig = _number(desc[idx])
            got, root = _device(eng, arena, arena_sz, d, nsig, keys)
            np.testing.assert_array_equal(got, want[idx], err_msg=str(cnt))
            np.testing.assert_array_equal(root, want_root[idx], err_msg=str(cnt))
            got, root = _registered(eng, arena, arena_sz, desc[idx], keys)
            np.testing.assert_array_equal(got, want[idx], err_msg=str(cnt))
            np.testing.assert_array_equal(root, want_root[idx], err_msg=str(cnt))
    finally:
        eng.close()
    # the host form in chunks: a context that holds a few records, fewer signature slots and two staged shreds
    eng = _engine(5, payload=2 * 1232 + 100, shreds=7, keys=4)
    try:
        for f in (_registered, _plain):
            got, root = f(eng, arena, arena_sz, desc[:40], keys)
            np.testing.assert_array_equal(got, want[:40])
            np.testing.assert_array_equal(root, want_root[:40])
    finally:
        eng.close()


def test_built_shreds():
    """Every depth 0-9 of all six kinds at leaf 0, 2^d - 1 and 2^d, with and without STRICT_LEAF; leaf 511 and 512;
    every alignment of off mod 8; a shred ending at the arena's last byte; record counts around a wavefront and a
    block; the host form's chunks"""
    _built()


# ---- 3: one signature per FEC set ----------------------------------------------------------------------------

@_once
def _mixed():
    g = fixture()
    shreds = [g["shreds"][i, :g["shred_sz"][i]].tobytes() for i in range(186)]
    arena, arena_sz, desc = _place(shreds, seed=13)
    seen = {}
    for i, s in enumerate(shreds):
        if s[:64] not in seen:
            seen[s[:64]] = i
            desc[i]["key_idx"] = g["shred_key"][i]
    first = sorted(seen.values())
    assert len(first) == 5
    roots = g["c_root"][:186]
    zero = np.zeros(186, np.int8)
    eng = _engine(256, payload=186 * 1232, shreds=186, keys=5)
    try:
        d, nsig = _number(desc)
        assert nsig == 5
        got, root = _device(eng, arena, arena_sz, d, nsig, g["keys"])
        np.testing.assert_array_equal(got, zero)
        np.testing.assert_array_equal(root, roots)
        got, root = _device(eng, arena, arena_sz, d, nsig, g["keys"], want_root=False)
        np.testing.assert_array_equal(got, zero)
        for f in (_registered, _plain):
            got, root = f(eng, arena, arena_sz, desc, g["keys"])
            np.testing.assert_array_equal(got, zero)
            np.testing.assert_array_equal(root, roots)
            got, root = f(eng, arena, arena_sz, desc, g["keys"], want_root=False)
            np.testing.assert_array_equal(got, zero)
            assert root is None
        # the set's members share its root: what the resolver compares on the host
        for i, s in enumerate(shreds):
            assert roots[i].tobytes() == roots[seen[s[:64]]].tobytes()
        # a set under the wrong leader: its keyed shred alone says so
        bad = d.copy()
        bad[first[2]]["key_idx"] = 1 - int(g["shred_key"][first[2]])
        got, root = _device(eng, arena, arena_sz, bad, nsig, g["keys"])
        i = first[2]
        wrong = ks._oracle().verify(roots[i].tobytes(), shreds[i][:64], g["keys"][bad[i]["key_idx"]].tobytes(), 0)
        assert wrong != 0 and got[i] == wrong, (got[i], wrong)
        got[i] = 0
        np.testing.assert_array_equal(got, zero)
        # no signature at all: roots only, no verify kernel
        none = desc.copy()
        none["key_idx"] = NO_SIG
        got, root = _device(eng, arena, arena_sz, none, 0, g["keys"][:0])
        np.testing.assert_array_equal(got, zero)
        np.testing.assert_array_equal(root, roots)
        got, root = _plain(eng, arena, arena_sz, none, g["keys"][:0])
        np.testing.assert_array_equal(got, zero)
        np.testing.assert_array_equal(root, roots)
    finally:
        eng.close()


def test_mixed_batch():
    """The resolver's call over the fixture: the first shred of each of the five FEC sets carries the key, the other
    181 are NO_SIG; sig_cnt = 0; roots for every record, and none asked for"""
    _mixed()


# ---- 4: bad descriptors ---------------------------------------------------------------------------------------

@_once
def _bad_descriptors():
    o = ks._oracle()
    shreds = [bytearray(sm.build(KINDS[t % 6], 3 + t % 5, 1 + t % 5, 500 + t, lambda r: ks._sign(t % 2, r)[0])) for t in range(8)]
    shreds[3][40] ^= 1
    shreds = [bytes(s) for s in shreds]
    arena, A, good = _place(shreds, seed=14, last_flush=True)
    keys = np.frombuffer(ks._key(0)[0] + ks._key(1)[0], np.uint8).reshape(2, 32)
    good["key_idx"] = [t % 2 for t in range(8)]
    want8 = [o.verify(sm.outcome(s, len(s))[1], s[:64], keys[t % 2].tobytes(), 0) for t, s in enumerate(shreds)]
    root8 = [sm.outcome(s, len(s))[1] for s in shreds]
    assert want8[3] != 0 and want8.count(0) == 7
    g0 = good[0]
    # (off, sz, key_idx, sig_idx): a range past the arena three ways, a key past the keys two ways, a slot past the
    # slots two ways (sig_idx is set after the numbering below)
    bad = [(A - 1202, 1203, 0, None), (0xFFFFFFFF, 0xFFFF, NO_SIG, None), (A, 1, 1, None), (g0["off"], 1203, 2, None),
           (g0["off"], 1203, 0xFFFE, None), (g0["off"], 1203, 0, "cnt"), (g0["off"], 1203, 0, 0xFFFFFFFF)]
    rows, want, roots, slot_bad = [], [], [], []
    for i in range(8):
        rows.append(tuple(good[i]))
        want.append(want8[i])
        roots.append(root8[i])
        if i < len(bad):
            off, sz, key, sig = bad[i]
            rows.append((off, sz, key, 0, 0))
            want.append(DESC)
            roots.append(bytes(32))
            slot_bad.append((len(rows) - 1, sig))
    desc = np.array(rows, engine.SHRED_DESC_DTYPE)
    want, roots = np.array(want, np.int8), np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32)
    d, nsig = _number(desc)
    for i, sig in slot_bad:
        if sig is not None:
            d[i]["sig_idx"] = nsig if sig == "cnt" else sig
    eng = _engine(64, payload=16 * 1232, shreds=len(desc), keys=2)
    try:
        got, root = _device(eng, arena, A, d, nsig, keys)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(root, roots)
        # the host form numbers the slots itself, so there the last two are good records: shred 0 under key 0
        hw, hr = want.copy(), roots.copy()
        hw[[11, 13]], hr[[11, 13]] = want8[0], np.frombuffer(root8[0], np.uint8)
        for f in (_registered, _plain):
            got, root = f(eng, arena, A, desc, keys)
            np.testing.assert_array_equal(got, hw)
            np.testing.assert_array_equal(root, hr)
        # one byte less, one key less, one slot less: good
        edge = np.array([(A - 1203, 1203, 1, 0, 0), (int(g0["off"]), 1203, 1, 1, 0), (int(g0["off"]), 1203, 0, 2, 0)],
                        engine.SHRED_DESC_DTYPE)
        got, root = _device(eng, arena, A, edge, 3, keys)
        other = o.verify(root8[0], shreds[0][:64], keys[1].tobytes(), 0)
        assert got[0] == want8[7] == 0 and got[2] == want8[0] == 0 and got[1] == other != 0, got
    finally:
        eng.close()


def test_bad_descriptors():
    """Seven bad descriptors, each between two good records, which keep their codes and roots"""
    _bad_descriptors()


# ---- 5: refusals ----------------------------------------------------------------------------------------------

@_once
def _refusals():
    shreds = [sm.build(0x90, 5, t, 700 + t, lambda r: ks._sign(0, r)[0]) for t in range(12)]
    arena, A, desc = _place(shreds, seed=15)
    desc["key_idx"] = 0
    keys = np.frombuffer(ks._key(0)[0], np.uint8).reshape(1, 32)
    keys3 = np.concatenate([keys, keys, keys])
    d, nsig = _number(desc)
    zero = np.zeros(12, np.int8)
    eng = _engine(8, payload=16 * 1232)
    try:
        # unprepared
        assert _refused(_device, eng, arena, A, d, nsig, keys) == -3
        assert _refused(_registered, eng, arena, A, desc, keys) == -3
        assert _refused(_plain, eng, arena, A, desc, keys) == -3
        assert _refused(eng.shreds_prepare, 0, 1) == -1
        assert _refused(eng.shreds_prepare, 12, 0) == -1
        assert _refused(eng.shreds_prepare, 12, 0x10000) == -1
        eng.shreds_prepare(12, 2)
        # 12 records fit, 12 signatures do not: the context has 8 slots
        assert _refused(_device, eng, arena, A, d, nsig, keys) == -1
        assert _refused(_device, eng, arena, A, d[:8], 8, keys3) == -1          # 3 keys, 2 prepared
        assert _refused(_registered, eng, arena, A, desc, keys3) == -1
        got, _ = _device(eng, arena, A, d[:8], 8, keys)
        np.testing.assert_array_equal(got, zero[:8])
        big = np.concatenate([desc, desc])
        big["key_idx"][8:] = NO_SIG
        db, nb = _number(big)
        assert _refused(_device, eng, arena, A, db, nb, keys) == -1             # 24 records, 12 prepared
        # the host form cuts chunks instead
        for f in (_registered, _plain):
            np.testing.assert_array_equal(f(eng, arena, A, np.concatenate([desc, desc]), keys)[0], np.concatenate([zero, zero]))
        # a smaller size changes nothing, a larger one reallocates
        eng.shreds_prepare(4, 1)
        np.testing.assert_array_equal(_device(eng, arena, A, db[:12], 8, keys)[0], zero)
        eng.shreds_prepare(24, 3)
        np.testing.assert_array_equal(_device(eng, arena, A, db, nb, keys3)[0], np.concatenate([zero, zero]))
        # the async pipeline holds a transaction: the synchronous calls' refusal
        sig, pub = ks._sign(0, b"x" * 40)
        assert eng.submit(sig + pub + b"x" * 40, 0, 64, 96, 1, 7) == 0
        assert _refused(_registered, eng, arena, A, desc, keys) == -1
        assert _refused(_plain, eng, arena, A, desc, keys) == -1
        eng.flush()
        tags, codes = eng.poll(blocking=True)
        assert list(tags) == [7] and list(codes) == [0]
        np.testing.assert_array_equal(_plain(eng, arena, A, desc, keys)[0], zero)
        # a faulted context
        eng.debug_fault()
        assert _refused(_device, eng, arena, A, d[:8], 8, keys) == -3
        assert _refused(_plain, eng, arena, A, desc, keys) == -3
        assert _refused(eng.shreds_prepare, 100, 1) == -3
    finally:
        eng.close()
    # no staging: the device form and a registered arena work, any other memory is refused
    eng = _engine(16, shreds=12, keys=1)
    try:
        np.testing.assert_array_equal(_device(eng, arena, A, d, nsig, keys)[0], zero)
        np.testing.assert_array_equal(_registered(eng, arena, A, desc, keys)[0], zero)
        assert _refused(_plain, eng, arena, A, desc, keys) == -3
    finally:
        eng.close()


def test_refusals():
    _refusals()


# ---- 6: pins reach these callers ------------------------------------------------------------------------------

@_once
def _pins():
    who = []
    for c in range(40):                                       # 40 cold leaders, one shred each, among 4 x 15 pinned
        who.append(100 + c)
        who += [(3 * c + j) % 4 for j in range(3)] if c < 20 else []
    assert len(who) == 100 and all(who.count(p) == 15 for p in range(4))
    leaders = sorted(set(who))
    shreds = [bytearray(sm.build(KINDS[i % 6], 6, 1 + i % 60, 900 + i, lambda r: ks._sign(kk, r)[0])) for i, kk in enumerate(who)]
    shreds[1][70] ^= 2
    shreds = [bytes(s) for s in shreds]
    extra = [sm.build(0x90, 6, i, 1200 + i, lambda r: bytes(64)) for i in range(28)]          # roots only
    arena, A, desc = _place(shreds + extra, seed=16)
    desc["key_idx"][:100] = [leaders.index(kk) for kk in who]
    keys = np.frombuffer(b"".join(ks._key(kk)[0] for kk in leaders), np.uint8).reshape(-1, 32)
    want = np.zeros(128, np.int8)
    want[1] = ks._oracle().verify(sm.outcome(shreds[1], 1203)[1], shreds[1][:64], ks._key(who[1])[0], 0)
    assert want[1] != 0
    d, nsig = _number(desc)
    eng = _engine(4096, shreds=128, keys=len(keys), half=1, small_batch_max=0)
    try:
        eng.set_pinned_keys([ks._key(p)[0] for p in range(4)])
        got, _ = _device(eng, arena, A, d, nsig, keys)
        np.testing.assert_array_equal(got, want)
        assert eng.pinned_count() == (4, 60), eng.pinned_count()
    finally:
        eng.close()


def test_pins_reach_these_callers():
    """Four pinned leaders with 15 keyed shreds each on the throughput path, among 40 other leaders and 28 NO_SIG"""
    _pins()


# ---- 7: batch SHA-256 -----------------------------------------------------------------------------------------

SHA_SIZES = (0, 1, 3, 4, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 1045, 1203, 4096)


@_once
def _sha256():
    import torch
    msgs, offs, buf = [], [], bytearray()
    for n in SHA_SIZES:
        for mod in range(4):
            buf += b"\xA5" * ((mod - len(buf)) % 4 + 4)
            offs.append(len(buf))
            msgs.append(hashlib.shake_256(b"sha256 %d %d" % (n, mod)).digest(n) if n else b"")
            buf += msgs[-1]
    assert [o % 4 for o in offs[:4]] == [0, 1, 2, 3]
    want = np.frombuffer(b"".join(hashlib.sha256(m).digest() for m in msgs), np.uint8).reshape(-1, 32)
    data = torch.from_numpy(np.frombuffer(bytes(buf) + b"\xEE" * 128, np.uint8).copy()).cuda()
    off = torch.from_numpy(np.array(offs, np.uint64).view(np.int64)).cuda()
    sz = torch.from_numpy(np.array([len(m) for m in msgs], np.uint32).view(np.int32)).cuda()
    out = torch.zeros((len(msgs), 32), dtype=torch.uint8, device="cuda")
    engine.sha256_batch_device(data.data_ptr(), off.data_ptr(), sz.data_ptr(), len(msgs), out.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    got = engine.sha256_batch_host(msgs)
    assert got == [hashlib.sha256(m).digest() for m in msgs]
    assert engine.sha256_batch_host([]) == []


def test_sha256_batch():
    """Sizes around a word, the padding's edge (55 / 56), a block and two, a shred's leaf and 4,096, each at all four
    offsets mod 4, through the device form and the host form, against hashlib"""
    _sha256()
