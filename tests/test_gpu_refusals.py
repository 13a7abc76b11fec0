"""GPU: what the engine's host entry points refuse, one condition at a time.

* The synchronous calls (fdgpu_ed25519_verify_txns_host, _verify_many_host, _verify_txn_ptrs,
  _verify_raw_host): a malformed batch, a batch or record larger than the context, a context without
  staging buffers, and a context whose async pipeline holds a record -- each with its result code and
  its fdgpu_last_error text.
* The gathered submits (fdgpu_ed25519_submit_raw_gather_chk, _dev, _dev_f, _to): the record check of
  each (sizes, the 16-byte alignment of the source and the destination, the 8-byte alignment of the seq
  word, the footprint-offset rule, the flags each admits), and that a refused record leaves nothing in
  the pipeline.
* fdgpu_ed25519_verify_txns_host reading the payload straight from pinned memory gives the codes it
  gives through the staging slot, and the oracle's.

Every context is 64 transactions / 64 signatures; apart from the last test only the kernels of context
creation run.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_vp, _us, _ul, _ui = ctypes.c_void_p, ctypes.c_ushort, ctypes.c_ulong, ctypes.c_uint
REGION = 1 << 14


def _lib():
    from firedancer_amd import engine
    L = engine.load_library()
    L.fdgpu_ed25519_submit_raw_gather_dev.restype = ctypes.c_int
    L.fdgpu_ed25519_submit_raw_gather_dev.argtypes = [_vp, _vp, _vp, _vp, _vp, _us, _us, _us, _ul, _vp, _ul]
    L.fdgpu_ed25519_submit_raw_gather_dev_f.restype = ctypes.c_int
    L.fdgpu_ed25519_submit_raw_gather_dev_f.argtypes = [_vp, _vp, _vp, _vp, _vp, _us, _us, _us, _ul, _vp, _ul, _ui]
    L.fdgpu_ed25519_submit_raw_gather_to.restype = ctypes.c_int
    L.fdgpu_ed25519_submit_raw_gather_to.argtypes = [_vp, _vp, _vp, _vp, _us, _us, _us, _ul, _vp, _ul, _ui]
    return L


def _engine(max_payload=1 << 16):
    from firedancer_amd import engine
    return engine.Engine(device=0, max_txn=64, max_sig=64, max_payload=max_payload)


def _idle(L, eng):
    f, i = ctypes.c_ulong(7), ctypes.c_ulong(7)
    L.fdgpu_ed25519_pipeline_state(eng.ctx, ctypes.byref(f), ctypes.byref(i))
    return f.value == 0 and i.value == 0


def _descs(n, payload_sz=200):
    """n single-signer descriptors over consecutive payload_sz-byte payloads"""
    from firedancer_amd import engine
    d = np.zeros(n, engine.DESC_DTYPE)
    d["payload_off"] = np.arange(n) * payload_sz
    d["sig_base"] = np.arange(n)
    d["payload_sz"] = payload_sz
    d["signature_off"], d["acct_addr_off"], d["message_off"], d["sig_cnt"] = 1, 69, 101, 1
    return d


# ---- the synchronous calls ------------------------------------------------------------------------------

def _txns_host(L, eng, payload, desc, n=None):
    n = len(desc) if n is None else n
    out = np.zeros(max(n, 1), np.int8)
    return L.fdgpu_ed25519_verify_txns_host(eng.ctx, payload.ctypes.data, payload.nbytes, desc.ctypes.data, n,
                                            out.ctypes.data, None)


def _many_host(L, eng, msg_sz):
    msg, sig, pub = np.zeros(msg_sz + 1, np.uint8), np.zeros(64, np.uint8), np.zeros(32, np.uint8)
    ptr = [np.array([a.ctypes.data], np.uint64) for a in (msg, sig, pub)]
    szs, out = np.array([msg_sz], np.uint64), np.zeros(1, np.int8)
    return L.fdgpu_ed25519_verify_many_host(eng.ctx, ptr[0].ctypes.data, szs.ctypes.data, ptr[1].ctypes.data,
                                            ptr[2].ctypes.data, 1, out.ctypes.data)


def _txn_ptrs(L, eng, payload_sz):
    buf, desc, out = np.zeros(payload_sz + 1, np.uint8), _descs(1, payload_sz), np.zeros(1, np.int8)
    ptr = np.array([buf.ctypes.data], np.uint64)
    return L.fdgpu_ed25519_verify_txn_ptrs(eng.ctx, ptr.ctypes.data, desc.ctypes.data, 1, out.ctypes.data)


def _raw_host(L, eng, payload, off, sz, img_stride=None):
    from firedancer_amd import engine
    n = len(off)
    raw = np.zeros(n, engine.RAW_DTYPE)
    raw["payload_off"], raw["payload_sz"] = off, sz
    out, fp = np.zeros(n, np.int8), np.zeros(n, np.uint16)
    img = np.zeros((n, engine.TXN_IMG_STRIDE), np.uint8) if img_stride else None
    return L.fdgpu_ed25519_verify_raw_host(eng.ctx, payload.ctypes.data, payload.nbytes, raw.ctypes.data, n,
                                           out.ctypes.data, img.ctypes.data if img_stride else None,
                                           img_stride or engine.TXN_IMG_STRIDE, fp.ctypes.data)


def test_verify_txns_host_refusals():
    from firedancer_amd import engine
    L, eng = _lib(), _engine()
    payload = np.zeros(400, np.uint8)
    d = _descs(2)
    d["sig_base"][1] = 2
    assert _txns_host(L, eng, payload, d) == -1
    assert engine.last_error() == "sig_base is not the prefix sum of sig_cnt"
    d = _descs(2)
    d["payload_sz"][1] = 201
    assert _txns_host(L, eng, payload, d) == -1
    assert engine.last_error() == "payload out of arena"
    assert _txns_host(L, eng, np.zeros(65 * 200, np.uint8), _descs(65)) == -1
    assert engine.last_error() == "batch larger than ctx"
    assert _txns_host(L, eng, payload, _descs(2), n=0) == 0
    assert _idle(L, eng)
    eng.close()


@pytest.mark.parametrize("call", [_many_host, _txn_ptrs])
def test_chunked_calls_refusals(call):
    from firedancer_amd import engine
    L = _lib()
    eng = _engine(max_payload=0)
    assert call(L, eng, 200) == -3
    assert engine.last_error() == "ctx has no staging buffers (max_payload_bytes==0)"
    eng.close()
    eng = _engine(max_payload=1024)
    assert call(L, eng, 1020) == -1          # a record longer than the arena
    assert engine.last_error() == ("message too long" if call is _many_host else "transaction larger than the ctx")
    assert _idle(L, eng)
    eng.close()


def test_verify_raw_host_refusals():
    from firedancer_amd import engine
    L, eng = _lib(), _engine()
    payload = np.zeros(400, np.uint8)
    assert _raw_host(L, eng, payload, [0, 200], [200, 201]) == -1
    assert engine.last_error() == "payload out of arena"
    assert _raw_host(L, eng, payload, [0, 200], [200, 200], img_stride=851) == -1
    assert engine.last_error() == "img_stride < FD_TXN_MAX_SZ"
    assert _idle(L, eng)
    eng.close()


@pytest.mark.parametrize("call", ["txns_host", "many_host", "txn_ptrs", "raw_host"])
def test_sync_calls_refuse_while_a_record_is_pending(call):
    from firedancer_amd import engine
    L, eng = _lib(), _engine()
    assert eng.submit_raw(bytes(200), 1) == 0          # submitted, not flushed
    payload = np.zeros(400, np.uint8)
    rc = {"txns_host": lambda: _txns_host(L, eng, payload, _descs(2)),
          "many_host": lambda: _many_host(L, eng, 200),
          "txn_ptrs": lambda: _txn_ptrs(L, eng, 200),
          "raw_host": lambda: _raw_host(L, eng, payload, [0, 200], [200, 200])}[call]()
    assert rc == -1
    assert engine.last_error() == "async batches pending or in flight"
    f, i = ctypes.c_ulong(), ctypes.c_ulong()
    L.fdgpu_ed25519_pipeline_state(eng.ctx, ctypes.byref(f), ctypes.byref(i))
    assert (f.value, i.value) == (1, 0)                # the pending record is untouched
    eng.close()


# ---- the gathered submits -------------------------------------------------------------------------------

class _Regions:
    """a source and an out region from fdgpu_host_alloc, with their device views"""

    def __init__(self, L):
        self.L = L
        self.src, self.out = L.fdgpu_host_alloc(REGION), L.fdgpu_host_alloc(REGION)
        assert self.src and self.out
        ctypes.memset(self.src, 0, REGION)
        self.src_dev, self.out_dev = L.fdgpu_host_dev_ptr(self.src, REGION), L.fdgpu_host_dev_ptr(self.out, REGION)
        assert self.src_dev and self.out_dev

    def free(self):
        self.L.fdgpu_host_free(self.src)
        self.L.fdgpu_host_free(self.out)


@pytest.fixture
def regions():
    r = _Regions(_lib())
    yield r
    r.free()


def _gather(L, eng, r, form, copy_sz=512, payload_off=16, payload_sz=200, src_skew=0, dst_skew=0, seq_skew=0,
            flags=None, src=None, dst_null=False):
    """one gathered submit in `form`; the seq word is the source region's last, the record 64 bytes into both"""
    s = (r.src + 64 if src is None else src) + src_skew
    s_dev = r.src_dev + 64 + src_skew
    seq, seq_dev = r.src + REGION - 8 + seq_skew, r.src_dev + REGION - 8 + seq_skew
    dst = r.out + 64 + dst_skew
    if form == "chk":
        return L.fdgpu_ed25519_submit_raw_gather_chk(eng.ctx, s, r.out, dst, copy_sz, payload_off, payload_sz, 9, seq, 0)
    if form == "dev":
        return L.fdgpu_ed25519_submit_raw_gather_dev(eng.ctx, s, s_dev, r.out, dst, copy_sz, payload_off, payload_sz, 9,
                                                     seq_dev, 0)
    if form == "dev_f":
        return L.fdgpu_ed25519_submit_raw_gather_dev_f(eng.ctx, s, s_dev, r.out, dst, copy_sz, payload_off, payload_sz,
                                                       9, seq_dev, 0, flags or 0)
    assert form == "to"
    return L.fdgpu_ed25519_submit_raw_gather_to(eng.ctx, s, s_dev, None if dst_null else r.out_dev + 64 + dst_skew,
                                                copy_sz, payload_off, payload_sz, 9, seq_dev, 0, flags or 0)


FORMS = ["chk", "dev", "dev_f", "to"]


def _bad_record(form):
    return "fdgpu_ed25519_submit_raw_gather%s: bad record" % ("_to" if form == "to" else "")


@pytest.mark.parametrize("form", FORMS)
def test_gather_record_check(form, regions):
    from firedancer_amd import engine
    L, eng = _lib(), _engine()
    for kw in (dict(copy_sz=215),        # payload_off + payload_sz = 216 > copy_sz
               dict(src_skew=8), dict(dst_skew=8), dict(seq_skew=4)):
        assert _gather(L, eng, regions, form, **kw) == -1, kw
        assert engine.last_error() == _bad_record(form)
        assert _idle(L, eng)
    # the footprint field lies in the record's header, ahead of the payload
    assert L.fdgpu_ed25519_set_record_fp_off(eng.ctx, 2) == 0
    for payload_off in (2, 256):
        assert _gather(L, eng, regions, form, payload_off=payload_off) == -1, payload_off
        assert engine.last_error() == _bad_record(form)
        assert _idle(L, eng)
    eng.close()


def test_gather_flags_and_places(regions):
    from firedancer_amd import engine
    L, eng = _lib(), _engine()
    assert _gather(L, eng, regions, "dev_f", flags=0x100) == -1      # a dedup seed: only the per-record form takes one
    assert engine.last_error() == _bad_record("dev_f")
    assert _idle(L, eng)
    assert _gather(L, eng, regions, "to", dst_null=True) == -1
    assert engine.last_error() == _bad_record("to")
    assert _idle(L, eng)
    outside = np.zeros(1024 + 16, np.uint8)
    src = (outside.ctypes.data + 15) & ~15
    assert _gather(L, eng, regions, "chk", src=src) == -3
    assert engine.last_error() == "fdgpu_ed25519_submit_raw_gather: src not in a registered region"
    assert _idle(L, eng)
    assert _gather(L, eng, regions, "to", flags=0x100) == 0          # a valid record with its seed: taken
    f, i = ctypes.c_ulong(), ctypes.c_ulong()
    L.fdgpu_ed25519_pipeline_state(eng.ctx, ctypes.byref(f), ctypes.byref(i))
    assert (f.value, i.value) == (1, 0)
    eng.close()


# ---- verify_txns_host from pinned memory ----------------------------------------------------------------

def test_verify_txns_host_pinned_payload(oracle):
    from firedancer_amd import synth
    L = _lib()
    payload, desc, expect, nsig = synth.make_batch(64, synth.SMALL_MSG, invalid_frac=0.25, seed=77)
    assert nsig == 64 and (expect != 0).any() and (expect == 0).any()
    o_txn, o_sig = oracle.verify_txns(payload, desc, nsig, threads=4)
    eng = _engine(max_payload=payload.nbytes)
    txn_a, sig_a = eng.verify_txns_host(payload, desc)
    p = L.fdgpu_host_alloc(payload.nbytes)
    assert p
    try:
        ctypes.memmove(p, payload.ctypes.data, payload.nbytes)
        pinned = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(payload.nbytes,))
        assert pinned.ctypes.data == p                   # the engine sees the pinned bytes themselves
        txn_b, sig_b = eng.verify_txns_host(pinned, desc)
    finally:
        L.fdgpu_host_free(p)
        eng.close()
    np.testing.assert_array_equal(txn_a, txn_b)
    np.testing.assert_array_equal(sig_a, sig_b)
    np.testing.assert_array_equal(txn_b, o_txn)
    np.testing.assert_array_equal(sig_b, o_sig)
    np.testing.assert_array_equal(txn_b, expect)
