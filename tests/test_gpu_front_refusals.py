"""GPU: what the descriptor front-ends and the two hash batches refuse, one table of
(context, call, return value, fdgpu_last_error text).

The nine entry points -- fdgpu_ed25519_sigs_prepare, _verify_sigs_device, _verify_sigs_host,
_shreds_prepare, _verify_shreds_device, _verify_shreds_host, _fec_prepare, _verify_fec_sets_device,
_verify_fec_sets_host -- and fdgpu_sha256_batch_host / fdgpu_sha512_batch_host (with the _device calls
behind them, which own "batch too large").  Every text was read from the source of the commit before the
front-ends' host code was folded; where two refusals apply at once, the row says which one wins.

"fdgpu_ed25519_verify_fec_sets_host: no signature slot" has no row: a chunk is empty only if the first set
finds no slot, fdgpu_ed25519_fec_prepare leaves at least one, and a set too large for a batch is refused
before the chunks start -- no argument reaches it.

The contexts are 64 transactions / 64 signatures, prepared with single-digit counts.  A refusal returns in
front of the call's first launch, so apart from context creation and the prepares no kernel runs.  Device
pointers are views of one zeroed fdgpu_host_alloc region all the same, never made-up numbers.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REGION = 1 << 14
ARENA_SZ = 4096                      # the arena is the region's first bytes, its slack behind it
OFF = dict(desc=8192, member=9216, keys=10240, expect=10496, root=10752, out=11776)
NO_SIG = 0xFFFF

FAULTED = "%s: the context has faulted"
BUSY = "async batches pending or in flight"
NO_STAGING = "ctx has no staging buffers (max_payload_bytes==0)"
KEYS_ROOT = "d_keys and d_root are 16-byte aligned"
KEYS_ROOT_EXPECT = "d_keys, d_root and d_expect are 16-byte aligned"


class _Mem:
    """one zeroed pinned region with its device view, and pageable arrays for the host forms"""

    def __init__(self, L):
        from firedancer_amd import engine
        self.L = L
        self.h = L.fdgpu_host_alloc(REGION)
        assert self.h
        ctypes.memset(self.h, 0, REGION)
        self.d = L.fdgpu_host_dev_ptr(self.h, REGION)
        assert self.d
        self.arena = np.zeros(ARENA_SZ + engine.ARENA_SLACK, np.uint8)
        self.sig = np.zeros(2, engine.SIG_DESC_DTYPE)              # two good records of 200 message bytes
        self.sig["pub_off"], self.sig["msg_off"], self.sig["msg_sz"] = 64, 96, 200
        self.long_sig = self.sig.copy()
        self.long_sig["msg_sz"][1] = 1000
        self.shred = np.zeros(2, engine.SHRED_DESC_DTYPE)
        self.shred["key_idx"] = NO_SIG
        self.fec = np.zeros(2, engine.FEC_DESC_DTYPE)              # two sets of one member each
        self.fec["member0"], self.fec["cnt"], self.fec["key_idx"] = [0, 1], 1, NO_SIG
        self.fec_root = self.fec.copy()
        self.fec_root["flags"][1] = engine.FDGPU_FEC_CHECK_ROOT
        self.fec_big = self.fec.copy()
        self.fec_big["cnt"][1] = 9                                  # members [1, 10) of 10: one more than prepared
        self.member = np.zeros(10, engine.FEC_MEMBER_DTYPE)
        self.keys = np.zeros(3 * 32, np.uint8)
        self.out = np.zeros(16, np.int8)
        self.root = np.zeros(16 * 32, np.uint8)
        self.huge = np.zeros((1 << 29) + 64, np.uint8)              # never touched: the refusal comes first

    def dev(self, name, skew=0):
        return self.d + OFF[name] + skew

    def free(self):
        self.L.fdgpu_host_free(self.h)


def _p(a):
    return None if a is None else a.ctypes.data


# ---- the calls: every argument has a good default, a row names what it changes -----------------------------

def _sigs_device(L, c, m, cnt=2, msg_bytes=400, arena=True, desc=True, out=True):
    return L.fdgpu_ed25519_verify_sigs_device(c, m.d if arena else None, ARENA_SZ, m.dev("desc") if desc else None, cnt,
                                              msg_bytes, m.dev("out") if out else None, None)


def _sigs_host(L, c, m, cnt=2, pinned=False, desc="sig", arena=True, out=True):
    a = (m.h if pinned else _p(m.arena)) if arena else None
    return L.fdgpu_ed25519_verify_sigs_host(c, a, ARENA_SZ, _p(getattr(m, desc)) if desc else None, cnt,
                                            _p(m.out) if out else None)


def _shreds_device(L, c, m, cnt=2, sig_cnt=0, key_cnt=1, arena=True, desc=True, keys=0, root=0, out=True):
    return L.fdgpu_ed25519_verify_shreds_device(c, m.d if arena else None, ARENA_SZ, m.dev("desc") if desc else None, cnt,
                                                sig_cnt, None if keys is None else m.dev("keys", keys), key_cnt,
                                                m.dev("out") if out else None,
                                                None if root is None else m.dev("root", root), None)


def _shreds_host(L, c, m, cnt=2, key_cnt=1, pinned=False, arena=True, desc=True, keys=True, out=True):
    a = (m.h if pinned else _p(m.arena)) if arena else None
    return L.fdgpu_ed25519_verify_shreds_host(c, a, ARENA_SZ, _p(m.shred) if desc else None, cnt,
                                              _p(m.keys) if keys else None, key_cnt, _p(m.out) if out else None, _p(m.root))


def _fec_device(L, c, m, set_cnt=2, member_cnt=2, sig_cnt=0, key_cnt=1, arena=True, desc=True, member=True, keys=0,
                expect=0, root=0, out=True):
    return L.fdgpu_ed25519_verify_fec_sets_device(c, m.d if arena else None, ARENA_SZ, m.dev("desc") if desc else None,
                                                  set_cnt, m.dev("member") if member else None, member_cnt, sig_cnt,
                                                  None if keys is None else m.dev("keys", keys), key_cnt,
                                                  None if expect is None else m.dev("expect", expect),
                                                  m.dev("out") if out else None,
                                                  None if root is None else m.dev("root", root), None)


def _fec_host(L, c, m, set_cnt=2, member_cnt=2, key_cnt=1, pinned=False, desc="fec", arena=True, member=True, keys=True,
              expect=False, out=True):
    a = (m.h if pinned else _p(m.arena)) if arena else None
    return L.fdgpu_ed25519_verify_fec_sets_host(c, a, ARENA_SZ, _p(getattr(m, desc)) if desc else None, set_cnt,
                                                _p(m.member) if member else None, member_cnt, _p(m.keys) if keys else None,
                                                key_cnt, _p(m.root) if expect else None, _p(m.out) if out else None,
                                                _p(m.root))


def _sha_host(which, data_sz=16, off=(0, 8), sz=(8, 8), cnt=2, huge=False):
    def call(L, c, m):
        o, s = np.array(off, np.uint64), np.array(sz, np.uint32)
        return getattr(L, "fdgpu_%s_batch_host" % which)(0, _p(m.huge if huge else m.arena), data_sz, _p(o), _p(s), cnt,
                                                         _p(m.root))
    return call


def _sha_device(which, cnt):
    def call(L, c, m):
        return getattr(L, "fdgpu_%s_batch_device" % which)(m.d, m.dev("desc"), m.dev("member"), cnt, m.dev("root"), None)
    return call


def _call(f, **kw):
    return lambda L, c, m: f(L, c, m, **kw)


def _prep(name, *a):
    return lambda L, c, m: getattr(L, "fdgpu_ed25519_%s_prepare" % name)(c, *a)


# ---- the contexts ------------------------------------------------------------------------------------------

def _prepared(eng):
    eng.sigs_prepare(4096)
    eng.shreds_prepare(8, 2)
    eng.fec_prepare(4, 8, 2)


def _make(kind):
    from firedancer_amd import engine
    if kind == "null":
        return None
    payload = {"nostage": 0, "small": 1024}.get(kind, 1 << 16)
    eng = engine.Engine(device=0, max_txn=64, max_sig=64, max_payload=payload)
    if kind in ("prep", "nostage", "small", "pending"):
        _prepared(eng)
    if kind == "tiny":
        eng.sigs_prepare(96)
    if kind == "pending":
        assert eng.submit_raw(bytes(200), 1) == 0          # submitted, not flushed
    if kind == "fault":
        _prepared(eng)
        eng.debug_fault()
    return eng


# ---- the table ---------------------------------------------------------------------------------------------
# context kinds: null (no context), fault (prepared, then fdgpu_ed25519_debug_fault), raw (nothing prepared),
# prep (sigs 4,096 bytes; shreds 8 records, 2 keys; FEC 4 sets, 8 members, 2 keys), tiny (sigs 96 bytes),
# nostage / small (prepared, max_payload 0 / 1,024), pending (prepared, one async record submitted)

def _rows():
    S, H, F = "fdgpu_ed25519_verify_sigs_", "fdgpu_ed25519_verify_shreds_", "fdgpu_ed25519_verify_fec_sets_"
    NINE = [("fdgpu_ed25519_sigs_prepare", _prep("sigs", 4096)), (S + "device", _sigs_device), (S + "host", _sigs_host),
            ("fdgpu_ed25519_shreds_prepare", _prep("shreds", 8, 2)), (H + "device", _shreds_device), (H + "host", _shreds_host),
            ("fdgpu_ed25519_fec_prepare", _prep("fec", 4, 8, 2)), (F + "device", _fec_device), (F + "host", _fec_host)]
    rows = []
    for name, f in NINE:
        rows.append((name + " NULL ctx", "null", f, -1, "NULL ctx"))
        rows.append((name + " faulted", "fault", f, -3, FAULTED % name))
    # an unprepared context; it wins over sizes, NULL arguments and alignment
    for name, f, prep in ((S + "device", _sigs_device, "sigs"), (H + "device", _shreds_device, "shreds"),
                          (H + "host", _shreds_host, "shreds"), (F + "device", _fec_device, "fec"), (F + "host", _fec_host, "fec")):
        text = "%s: no fdgpu_ed25519_%s_prepare" % (name, prep)
        rows.append((name + " unprepared", "raw", f, -3, text))
        rows.append((name + " unprepared, oversize, NULL", "raw", _call(f, key_cnt=99, arena=False) if f is not _sigs_device
                     else _call(f, cnt=99, arena=False), -3, text))
    rows.append((S + "host unprepared, in place", "raw", _call(_sigs_host, pinned=True), -3,
                 S + "host: no fdgpu_ed25519_sigs_prepare"))
    # the prepares' sizes
    for a in ((0,), (95,), ((1 << 32) - 511,)):
        rows.append(("sigs_prepare%r" % (a,), "raw", _prep("sigs", *a), -1, "fdgpu_ed25519_sigs_prepare: bad size"))
    for a in ((0, 1), (1 << 31, 1), (1, 0), (1, 0x10000)):
        rows.append(("shreds_prepare%r" % (a,), "raw", _prep("shreds", *a), -1, "fdgpu_ed25519_shreds_prepare: bad size"))
    for a in ((0, 1, 1), (1 << 31, 1, 1), (1, 0, 1), (1, 1 << 31, 1), (1, 1, 0), (1, 1, 0x10000)):
        rows.append(("fec_prepare%r" % (a,), "raw", _prep("fec", *a), -1, "fdgpu_ed25519_fec_prepare: bad size"))
    rows.append(("sigs_prepare again, smaller", "prep", _prep("sigs", 96), 0, None))
    rows.append(("shreds_prepare again, smaller", "prep", _prep("shreds", 1, 1), 0, None))
    rows.append(("fec_prepare again, smaller", "prep", _prep("fec", 1, 1, 1), 0, None))
    # sizes over the context's or the prepared ones; they win over an empty batch and over NULL arguments
    rows += [(S + "device cnt over ctx", "prep", _call(_sigs_device, cnt=65, arena=False), -1, "batch larger than ctx"),
             (S + "device msg_bytes over", "prep", _call(_sigs_device, cnt=0, msg_bytes=4097), -1,
              S + "device: 104 cnt + msg_bytes exceeds the prepared size"),
             (S + "device 104 cnt over", "prep", _call(_sigs_device, cnt=8, msg_bytes=4096 - 831, arena=False), -1,
              S + "device: 104 cnt + msg_bytes exceeds the prepared size"),
             (S + "device exactly full, empty", "prep", _call(_sigs_device, cnt=0, msg_bytes=4096, arena=False), 0, None),
             (H + "device cnt over", "prep", _call(_shreds_device, cnt=9, arena=False), -1, "batch larger than prepared"),
             (H + "device sig_cnt over", "prep", _call(_shreds_device, cnt=0, sig_cnt=9), -1, "batch larger than prepared"),
             (H + "device key_cnt over", "prep", _call(_shreds_device, key_cnt=3, keys=8), -1, "batch larger than prepared"),
             (H + "host key_cnt over", "prep", _call(_shreds_host, cnt=0, key_cnt=3, arena=False), -1, "more keys than prepared"),
             (F + "device set_cnt over", "prep", _call(_fec_device, set_cnt=5, arena=False), -1, "batch larger than prepared"),
             (F + "device member_cnt over", "prep", _call(_fec_device, set_cnt=0, member_cnt=9), -1, "batch larger than prepared"),
             (F + "device sig_cnt over", "prep", _call(_fec_device, sig_cnt=5, keys=8), -1, "batch larger than prepared"),
             (F + "device key_cnt over", "prep", _call(_fec_device, key_cnt=3), -1, "batch larger than prepared"),
             (F + "host key_cnt over", "prep", _call(_fec_host, set_cnt=0, key_cnt=3, arena=False), -1, "more keys than prepared")]
    # an empty batch is done, whatever its pointers
    rows += [(S + "device empty", "prep", _call(_sigs_device, cnt=0, msg_bytes=0, arena=False, desc=False, out=False), 0, None),
             (S + "host empty", "prep", _call(_sigs_host, cnt=0, arena=False, desc=None, out=False), 0, None),
             (H + "device empty", "prep", _call(_shreds_device, cnt=0, arena=False, desc=False, out=False, keys=8), 0, None),
             (H + "host empty", "prep", _call(_shreds_host, cnt=0, arena=False, desc=False, out=False), 0, None),
             (F + "device empty", "prep", _call(_fec_device, set_cnt=0, arena=False, desc=False, out=False, keys=8), 0, None),
             (F + "host empty", "prep", _call(_fec_host, set_cnt=0, arena=False, desc=None, out=False), 0, None)]
    # NULL arguments; they win over alignment
    for f, kws in ((_sigs_device, (dict(arena=False), dict(desc=False), dict(out=False))),
                   (_sigs_host, (dict(arena=False), dict(desc=None), dict(out=False))),
                   (_shreds_device, (dict(arena=False, keys=8), dict(desc=False), dict(out=False), dict(keys=None))),
                   (_shreds_host, (dict(arena=False), dict(desc=False), dict(out=False), dict(keys=False))),
                   (_fec_device, (dict(arena=False, root=8), dict(desc=False), dict(out=False), dict(member=False),
                                  dict(keys=None))),
                   (_fec_host, (dict(arena=False), dict(desc=None), dict(out=False), dict(member=False), dict(keys=False)))):
        for kw in kws:
            rows.append(("%s NULL %r" % (f.__name__, kw), "prep", _call(f, **kw), -1, "NULL argument"))
    rows += [(S + "host NULL, unprepared", "raw", _call(_sigs_host, out=False), -1, "NULL argument"),
             (H + "device no keys named", "prep", _call(_shreds_device, cnt=0, key_cnt=0, keys=None, root=None), 0, None)]
    # alignment
    rows += [(H + "device d_keys", "prep", _call(_shreds_device, keys=8), -1, KEYS_ROOT),
             (H + "device d_root", "prep", _call(_shreds_device, root=4), -1, KEYS_ROOT),
             (F + "device d_keys", "prep", _call(_fec_device, keys=8), -1, KEYS_ROOT_EXPECT),
             (F + "device d_root", "prep", _call(_fec_device, root=1), -1, KEYS_ROOT_EXPECT),
             (F + "device d_expect", "prep", _call(_fec_device, expect=8), -1, KEYS_ROOT_EXPECT)]
    # the host forms' own refusals
    rows += [(S + "host no staging", "nostage", _sigs_host, -3, NO_STAGING),
             (H + "host no staging", "nostage", _shreds_host, -3, NO_STAGING),
             (F + "host no staging", "nostage", _fec_host, -3, NO_STAGING),
             (S + "host long message", "small", _call(_sigs_host, desc="long_sig"), -1, "message too long"),
             (S + "host record over, in place", "tiny", _call(_sigs_host, pinned=True), -1,
              S + "host: a record larger than the prepared size"),
             (H + "host no shred fits", "small", _shreds_host, -1, "the staging slot holds no shred"),
             (F + "host CHECK_ROOT", "prep", _call(_fec_host, desc="fec_root"), -1, "FDGPU_FEC_CHECK_ROOT without expect"),
             (F + "host CHECK_ROOT, in place", "prep", _call(_fec_host, desc="fec_root", pinned=True), -1,
              "FDGPU_FEC_CHECK_ROOT without expect"),
             (F + "host set over", "prep", _call(_fec_host, desc="fec_big", member_cnt=10), -1,
              "a set holds more members than a batch may"),
             (F + "host set over, staged small", "small", _fec_host, -1, "a set holds more members than a batch may")]
    for name, f in ((S + "host", _sigs_host), (H + "host", _shreds_host), (F + "host", _fec_host)):
        rows.append((name + " pending", "pending", f, -1, BUSY))
        rows.append((name + " pending, in place", "pending", _call(f, pinned=True), -1, BUSY))
    # the hash batches
    for which in ("sha256", "sha512"):
        n = "fdgpu_%s_batch_" % which
        rows += [(n + "host empty", "null", _sha_host(which, cnt=0), 0, None),
                 (n + "host off over", "null", _sha_host(which, off=(0, 17), sz=(8, 0)), -1, "message out of buffer"),
                 (n + "host sz over", "null", _sha_host(which, off=(0, 8), sz=(8, 9)), -1, "message out of buffer"),
                 (n + "device empty", "null", _sha_device(which, 0), 0, None),
                 (n + "device over", "null", _sha_device(which, 1 << 31), -1, "batch too large")]
    rows.append(("fdgpu_sha256_batch_host 2^29", "null",
                 _sha_host("sha256", data_sz=(1 << 29) + 64, off=(0,), sz=(1 << 29,), cnt=1, huge=True), -1, "message out of buffer"))
    return rows


def test_front_refusals():
    from firedancer_amd import engine
    L = engine.load_library()
    L.fdgpu_ed25519_pipeline_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    m = _Mem(L)
    ctxs = {}
    try:
        for label, kind, call, rc, text in _rows():
            if kind not in ctxs:
                ctxs[kind] = _make(kind)
            eng = ctxs[kind]
            got = call(L, eng.ctx if eng else None, m)
            err = engine.last_error()
            print(label, got, repr(err))
            assert got == rc, (label, got, err)
            if text is not None:
                assert err == text, (label, err)
        # nothing was taken: the pending record is still the only one, the other contexts are idle
        for kind, eng in ctxs.items():
            if eng is None:
                continue
            f, i = ctypes.c_ulong(7), ctypes.c_ulong(7)
            L.fdgpu_ed25519_pipeline_state(eng.ctx, ctypes.byref(f), ctypes.byref(i))
            assert (f.value, i.value) == ((1, 0) if kind == "pending" else (0, 0)), kind
    finally:
        for eng in ctxs.values():
            if eng is not None:
                eng.close()
        m.free()
