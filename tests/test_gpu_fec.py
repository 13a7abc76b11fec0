"""GPU: whole FEC sets from descriptors (fdgpu_ed25519_verify_fec_sets_device / _host, DESIGN 23: fd_fec_tree_kernel
and fd_fec_flag_kernel around an unchanged batch).

Expected values never come from the code under test: the real sets' roots are the reference's recorded ones
(tests/golden/shreds.npz), the built sets' roots and proofs the reference's recorded trees (tests/golden/fec_trees.npz),
the codes of mutated sets tests/fec_model.py's, which tests/test_fec_desc.py holds against both fixtures, and the
signature codes the CPU oracle's.

test_real_sets_on_every_engine_path runs under the suite's engine-path parameter (tests/conftest.py).  The other
scenarios choose their options themselves, so they run on the GPU once (_once) and the suite's repeats only find
that they passed.
"""
import functools

import numpy as np
import pytest

from firedancer_amd import engine
from tests import fec_model as fm
from tests import shred_model as sm
from tests import test_gpu_key_split as ks
from tests.test_fec_desc import built_set, real_sets, trees
from tests.test_gpu_sigs import _Arena, _once, _refused
from tests.test_shred_desc import fixture

pytestmark = pytest.mark.gpu

DESC, MEMBER, ROOT, PROOF = engine.FDGPU_ERR_DESC, engine.FDGPU_ERR_FEC_MEMBER, engine.FDGPU_ERR_FEC_ROOT, engine.FDGPU_ERR_FEC_PROOF
NO_SIG, FILL = engine.FDGPU_SHRED_NO_SIG, engine.FDGPU_FEC_FILL
CHECK_ROOT, CHECK_PROOFS = engine.FDGPU_FEC_CHECK_ROOT, engine.FDGPU_FEC_CHECK_PROOFS
SLACK, GUARD = engine.ARENA_SLACK, 64


def _engine(n, payload=0, fec=None, keys=8, defaults=True, semantics=0, **opts):
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
    if fec:
        eng.fec_prepare(fec[0], fec[1], keys)
    return eng


def _signed(i, key):
    """set i of fec_trees.npz signed by key number key"""
    return built_set(i, lambda r: ks._sign(key, r)[0])


def _size(n):
    return fm.SIZES.index(n)


class _Batch:
    """Sets laid into one arena, member k at offset (5 k + k // 16) mod 16 behind a gap of junk (every alignment of a
    dword and a quad), and what the rules say of each"""

    def __init__(self, seed):
        self.ar, self.rows, self.members, self.sets = _Arena(seed), [], [], []

    def add(self, shreds, fill=(), flags=0, key=NO_SIG, expect=None):
        m0 = len(self.members)
        offs = []
        for j, s in enumerate(shreds):
            k = len(self.members)
            offs.append(self.ar.put(s, (5 * k + k // 16) % 16))
            self.members.append((offs[-1], FILL if j in fill else 0))
        self.rows.append((m0, len(shreds), key, 0, flags))
        self.sets.append(dict(shreds=list(shreds), fill=set(fill), flags=flags, key=key, expect=expect, offs=offs))
        return len(self.rows) - 1

    def raw(self, row, want, members=()):
        """a descriptor as given, over members as given, with the code it must get"""
        m0 = len(self.members)
        self.members += list(members)
        self.rows.append(tuple(row) if row[0] is not None else (m0,) + tuple(row[1:]))
        self.sets.append(dict(want=want))
        return len(self.rows) - 1

    def finish(self, last_flush=False):
        if not last_flush:
            self.ar.put(bytes(16))
        self.b = bytes(self.ar.b)
        self.A = len(self.b)
        self.desc = np.array(self.rows, engine.FEC_DESC_DTYPE)
        self.member = np.array(self.members, engine.FEC_MEMBER_DTYPE) if self.members else np.zeros(0, engine.FEC_MEMBER_DTYPE)
        return self

    def guarded(self):
        """(buffer, o): GUARD bytes, the arena page-aligned at o, its slack, GUARD bytes"""
        raw = np.zeros(self.A + SLACK + 3 * 4096, np.uint8)
        o = (-raw.ctypes.data) % 4096 + 4096
        raw[o - GUARD:o] = 0xC3
        raw[o:o + self.A] = np.frombuffer(self.b, np.uint8)
        raw[o + self.A:o + self.A + SLACK] = 0xEE
        raw[o + self.A + SLACK:o + self.A + SLACK + GUARD] = 0x3C
        return raw, o

    def want(self, keys, sem=0):
        """(codes, roots, the guarded bytes afterwards) by the model and the oracle"""
        o = ks._oracle()
        raw, at = self.guarded()
        codes, roots = [], []
        for s in self.sets:
            if "want" in s:
                codes.append(s["want"])
                roots.append(bytes(32))
                continue
            code, root, proofs = fm.outcome(s["shreds"], s["fill"], s["flags"], s["expect"])
            if not code:
                for j in s["fill"]:
                    m = s["offs"][j] + fm.moff(s["shreds"][j])
                    raw[at + m:at + m + len(proofs[j])] = np.frombuffer(proofs[j], np.uint8)
                if s["key"] != NO_SIG:
                    code = o.verify(root, s["shreds"][0][:64], bytes(keys[s["key"]]), sem)
            codes.append(code)
            roots.append(root if root is not None else bytes(32))
        view = raw[at - GUARD:at + self.A + SLACK + GUARD]
        return np.array(codes, np.int8), np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32), view.copy()


def _number(desc):
    d = desc.copy()
    keyed = d["key_idx"] != NO_SIG
    d["sig_idx"][keyed] = np.arange(int(keyed.sum()))
    return d, int(keyed.sum())


def _keys_array(keys):
    return np.ascontiguousarray(keys, np.uint8).reshape(-1, 32) if len(keys) else np.zeros((0, 32), np.uint8)


def _expects(b):
    if not any(s.get("expect") is not None for s in b.sets):
        return None
    return np.frombuffer(b"".join(s.get("expect") or bytes(32) for s in b.sets), np.uint8).reshape(-1, 32).copy()


def _device(eng, b, keys, desc=None, sig_cnt=None, want_root=True, expect="auto"):
    """(codes, roots, the guarded bytes afterwards) of the device form; desc / sig_cnt as numbered by the caller"""
    import torch
    if desc is None:
        desc, sig_cnt = _number(b.desc)
    raw, o = b.guarded()
    buf = torch.from_numpy(raw[o - GUARD:o + b.A + SLACK + GUARD].copy()).cuda()
    d = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).cuda()
    m = torch.from_numpy(np.ascontiguousarray(b.member).view(np.uint8).copy()).cuda() if len(b.member) else None
    keys = _keys_array(keys)
    k = torch.from_numpy(keys.reshape(-1).copy()).cuda() if len(keys) else None
    ex = _expects(b) if isinstance(expect, str) else expect
    e = torch.from_numpy(ex.reshape(-1).copy()).cuda() if ex is not None else None
    out = torch.full((len(desc),), 7, dtype=torch.int8, device="cuda")
    root = torch.full((len(desc), 32), 0x5A, dtype=torch.uint8, device="cuda") if want_root else None
    eng.verify_fec_sets_device(buf.data_ptr() + GUARD, b.A, d.data_ptr(), len(desc), m.data_ptr() if m is not None else None,
                               len(b.member), sig_cnt, k.data_ptr() if k is not None else None, len(keys),
                               e.data_ptr() if e is not None else None, out.data_ptr(),
                               root.data_ptr() if want_root else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (root.cpu().numpy() if want_root else None), buf.cpu().numpy()


def _host(eng, b, keys, registered, want_root=True, expect="auto"):
    raw, o = b.guarded()
    arena = raw[o:o + b.A + SLACK]
    ex = _expects(b) if isinstance(expect, str) else expect
    if registered:
        engine.host_register(arena)
    try:
        codes, roots = eng.verify_fec_sets_host(arena, b.desc, b.member, _keys_array(keys), ex, b.A, want_root)
    finally:
        if registered:
            engine.host_unregister(arena)
    return codes, roots, raw[o - GUARD:o + b.A + SLACK + GUARD].copy()


def _registered(eng, b, keys, **kw):
    return _host(eng, b, keys, True, **kw)


def _plain(eng, b, keys, **kw):
    return _host(eng, b, keys, False, **kw)


FORMS = (("device", _device), ("registered", _registered), ("plain", _plain))


def _all_forms(eng, b, keys, what, sem=0, forms=FORMS):
    codes, roots, after = b.want(keys, sem)
    for name, f in forms:
        got, root, bytes_after = f(eng, b, keys)
        np.testing.assert_array_equal(got, codes, err_msg=str((what, name, "codes")))
        np.testing.assert_array_equal(root, roots, err_msg=str((what, name, "roots")))
        assert bytes_after.tobytes() == after.tobytes(), (what, name, "arena", int((bytes_after != after).sum()))
    return codes, roots


# ---- 1: the real sets on every engine path ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _real_batch():
    b = _Batch(21)
    for shreds, root, key in real_sets():
        b.add(shreds, flags=CHECK_PROOFS, key=key)
    return b.finish(), fixture()["keys"], np.frombuffer(b"".join(r for _, r, _ in real_sets()), np.uint8).reshape(-1, 32)


def test_real_sets_on_every_engine_path(engine_path):
    """The five complete sets of the reference's archives (25, 33, 41, 23 and 64 leaves) with CHECK_PROOFS under their
    leaders: code 0 and the recorded roots in both semantics, through the device form and both host branches"""
    b, keys, roots = _real_batch()
    for sem in (engine.SEMANTICS_AVX512, engine.SEMANTICS_REF):
        eng = _engine(16, payload=186 * 1232, fec=(5, 186), keys=len(keys), defaults=False, semantics=sem)
        try:
            codes, got = _all_forms(eng, b, keys, (engine_path, sem), sem)
            assert not codes.any()
            np.testing.assert_array_equal(got, roots)
        finally:
            eng.close()


# ---- 2: FILL -----------------------------------------------------------------------------------------------

def _blank(shreds, which):
    out = list(shreds)
    for j in which:
        b, m = bytearray(out[j]), fm.moff(out[j])
        b[m:m + 20 * fm.depth(len(shreds))] = bytes(20 * fm.depth(len(shreds)))
        out[j] = bytes(b)
    return out


@_once
def _fill():
    g = trees()
    rng = np.random.default_rng(22)
    sets = [(built_set(i), g["root"][i].tobytes()) for i in range(len(fm.SIZES))] + [(s, r) for s, r, _ in real_sets()]
    b, whole = _Batch(22), _Batch(22)
    for shreds, root in sets:
        n = len(shreds)
        half = sorted(rng.choice(n, (n + 1) // 2, replace=False).tolist())
        for which in (half, list(range(n))):                   # the resolver's recovered half; the leader's whole set
            b.add(_blank(shreds, which), fill=which, flags=CHECK_ROOT | CHECK_PROOFS, expect=root)
            whole.add(shreds, flags=CHECK_ROOT | CHECK_PROOFS, expect=root)
    b.finish(), whole.finish()
    assert b.b != whole.b and b.A == whole.A
    roots = np.frombuffer(b"".join(r for _, r in sets for _ in range(2)), np.uint8).reshape(-1, 32)
    original = whole.guarded()
    original = original[0][original[1] - GUARD:original[1] + whole.A + SLACK + GUARD]
    eng = _engine(16, payload=300 * 1232, fec=(len(b.desc), len(b.member)))
    try:
        codes, _, after = b.want(())
        assert not codes.any() and after.tobytes() == original.tobytes()          # (the model fills what the builder wrote)
        for name, f in FORMS:
            got, root, bytes_after = f(eng, b, ())
            np.testing.assert_array_equal(got, codes, err_msg=name)
            np.testing.assert_array_equal(root, roots, err_msg=name)
            assert bytes_after.tobytes() == original.tobytes(), (name, int((bytes_after != original).sum()))
    finally:
        eng.close()


def test_fill_writes_the_reference_proofs():
    """Every n of the fixture and every real set, the proofs of a seeded half of the members zeroed and FILL on those,
    then all of them: the arena, its slack and 64 guard bytes on both sides equal the original byte for byte, the
    roots the reference's; the staged host branch in chunks of at most 300 members"""
    _fill()


# ---- 3: mixed sizes -----------------------------------------------------------------------------------------

@_once
def _mixed():
    keys = np.frombuffer(ks._key(0)[0] + ks._key(1)[0], np.uint8).reshape(2, 32)
    g = trees()
    order = (1, 2, 3, 33, 64, 65, 129, 256)
    eng = _engine(64, payload=600 * 1232, fec=(8, 553), keys=2)
    try:
        for sizes in (order, order[::-1]):
            b = _Batch(23)
            for t, n in enumerate(sizes):
                b.add(_signed(_size(n), t % 2), flags=CHECK_PROOFS | CHECK_ROOT, key=t % 2, expect=g["root"][_size(n)].tobytes())
            b.finish(last_flush=True)
            assert b.members[-1][0] + len(b.sets[-1]["shreds"][-1]) == b.A
            assert {off % 8 for off, _ in b.members} == set(range(8))
            codes, _ = _all_forms(eng, b, keys, sizes)
            assert not codes.any()
    finally:
        eng.close()


def test_mixed_sizes_in_one_batch():
    """Sets of 1, 2, 3, 33, 64, 65, 129 and 256 leaves in one batch, in that order and in reverse: small sets in blocks
    sized for 256; every alignment of off mod 8; a code shred and a data shred ending at the arena's last byte"""
    _mixed()


@_once
def _many():
    g = trees()
    order = (1, 2, 3, 33, 64, 65, 129, 256)
    b = _Batch(33)
    for n in order:
        b.add(built_set(_size(n)), flags=CHECK_PROOFS | CHECK_ROOT, expect=g["root"][_size(n)].tobytes())
    b.finish()
    # 2,100 descriptors over those eight sets' members, a bad one after every seven
    bad = ((0, 0, NO_SIG, 0, 0), (0, 257, NO_SIG, 0, 0), (500, 200, NO_SIG, 0, 0), (0xFFFFFFFF, 64, NO_SIG, 0, 0), (0, 64, 0, 0, 0))
    rows, want, roots, expect = [], [], [], []
    for t in range(2100):
        if t % 8 == 7:
            rows.append(bad[(t // 8) % len(bad)])
            want.append(DESC)
            roots.append(bytes(32))
            expect.append(bytes(32))
        else:
            k = (t + t // 8) % 8
            rows.append(b.rows[k])
            want.append(0)
            roots.append(g["root"][_size(order[k])].tobytes())
            expect.append(roots[-1])
    desc = np.array(rows, engine.FEC_DESC_DTYPE)
    expect = np.frombuffer(b"".join(expect), np.uint8).reshape(-1, 32).copy()
    eng = _engine(16, fec=(2100, len(b.member)))
    try:
        got, root, after = _device(eng, b, (), desc, 0, expect=expect)
        np.testing.assert_array_equal(got, np.array(want, np.int8))
        np.testing.assert_array_equal(root, np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32))
        assert after.tobytes() == b.want(())[2].tobytes()
    finally:
        eng.close()


def test_more_sets_than_are_resident_at_once():
    """2,100 sets of 1 ... 256 leaves with bad descriptors among them through the device form, which then launches once
    per block size: every set is taken by exactly one launch, the bad ones too"""
    _many()


# ---- 4: each code -------------------------------------------------------------------------------------------

def _with(shreds, j, off, new):
    out = list(shreds)
    b = bytearray(out[j])
    b[off:off + len(new)] = new
    out[j] = bytes(b)
    return out


def _xor(shreds, j, off, bit=1):
    return _with(shreds, j, off, bytes([shreds[j][off] ^ bit]))


@_once
def _member_rules():
    """one mutated field in one member -- first, middle and last of its kind -- per rule"""
    base = {cls: fm.build_set(5, 4, cls, 77 + cls, lambda r: ks._sign(0, r)[0]) for cls in (0, 1, 2)}
    keys = np.frombuffer(ks._key(0)[0], np.uint8).reshape(1, 32)
    b = _Batch(24)
    good = [b.add(base[cls], flags=CHECK_PROOFS, key=0) for cls in (0, 1, 2)]
    bad = []

    def case(shreds, what):
        assert fm.member_error(shreds), what
        bad.append((b.add(shreds, flags=CHECK_PROOFS, key=0), what))

    for cls in (1, 2):
        s = base[cls]
        D = fm.depth(9)
        for j in (0, 2, 4, 5, 7, 8):
            data = j < 5
            case(_xor(s, j, 0x41), ("slot", cls, j))
            case(_xor(s, j, 0x4d), ("version", cls, j))
            case(_xor(s, j, 0x4e, 0x80), ("version high", cls, j))
            if j:
                case(_xor(s, j, 0x4f), ("fec_set_idx", cls, j))      # (a data member's leaf moves with it)
                case(_xor(s, j, 0x30, 0x10), ("signature", cls, j))
                case(_xor(s, j, fm.moff(s[j]) - 32 + j), ("chained root", cls, j))
            case(_with(s, j, 0x40, bytes([(s[j][0x40] & 0xf0) | (D + 1)])), ("depth", cls, j))
            case(_with(s, j, 0x40, bytes([(s[j][0x40] & 0xf0) | (D - 1)])), ("depth", cls, j))
            other = fm.CLASSES[3 - cls][0 if data else 1]          # chained <-> resigned, same kind
            case(_with(s, j, 0x40, bytes([other | D])), ("type", cls, j))
            case(_with(s, j, 0x40, bytes([0xa0 | D])), ("legacy", cls, j))
            if data:
                case(_with(s, j, 0x49, (int.from_bytes(s[j][0x4f:0x53], "little") + j + 1).to_bytes(4, "little")), ("leaf", cls, j))
                if j:
                    case(_with(s, j, 0x53, (3 + (77 + cls) % 7).to_bytes(2, "little")), ("parent_off", cls, j))
                case(_with(s, j, 0x56, (87).to_bytes(2, "little")), ("parse: size", cls, j))
            else:
                case(_with(s, j, 0x55, (5).to_bytes(2, "little")), ("code_cnt: the sum", cls, j))
                if j > 5:
                    case(_with(s, j, 0x53, (6).to_bytes(2, "little") + (3).to_bytes(2, "little") + (j - 6).to_bytes(2, "little")),
                         ("data_cnt against the first code member", cls, j))
                case(_with(s, j, 0x57, ((j - 5 + 1) % 4).to_bytes(2, "little")), ("leaf", cls, j))
        # a code shred as leaf 0; two members swapped; one member short
        case([s[5]] + s[1:], ("code in front", cls))
        case(s[:2] + [s[3], s[2]] + s[4:], ("swapped", cls))
        case(s[:8], ("short", cls))
    good.append(b.add(base[1], flags=CHECK_PROOFS, key=0))
    b.finish()
    eng = _engine(256, payload=len(b.member) * 1232, fec=(len(b.desc), len(b.member)), keys=1)
    try:
        codes, roots = _all_forms(eng, b, keys, "member rules")
        assert all(codes[i] == 0 for i in good) and all(codes[i] == MEMBER for i, _ in bad), \
            [w for i, w in bad if codes[i] != MEMBER]
        assert not roots[[i for i, _ in bad]].any() and len(bad) > 100
    finally:
        eng.close()


def test_member_rules():
    _member_rules()


@_once
def _other_codes():
    o = ks._oracle()
    keys = np.frombuffer(ks._key(0)[0] + ks._key(1)[0], np.uint8).reshape(2, 32)
    g = trees()
    i33, i9 = _size(33), _size(9)
    s33, s9 = _signed(i33, 0), _signed(i9, 1)
    r33, r9 = g["root"][i33].tobytes(), g["root"][i9].tobytes()
    m = fm.moff(s33[20])
    b = _Batch(25)
    want = {}

    def add(code, *a, **kw):
        want[b.add(*a, **kw)] = code

    add(0, s33, flags=CHECK_ROOT | CHECK_PROOFS, key=0, expect=r33)
    add(ROOT, s33, flags=CHECK_ROOT | CHECK_PROOFS, key=0, expect=r9)                         # a wrong expect
    add(0, s9, flags=CHECK_ROOT, key=1, expect=r9)
    flipped = _xor(s33, 20, m + 45, 0x08)
    add(PROOF, flipped, flags=CHECK_PROOFS, key=0)                                             # one proof byte
    add(0, flipped, fill={20}, flags=CHECK_PROOFS, key=0)                                      # ... rewritten under FILL
    add(0, flipped, key=0)                                                                     # ... not looked at
    add(0, flipped, flags=CHECK_ROOT, key=0, expect=r33)
    body = _xor(s33, 3, 300, 0x40)
    add(ROOT, body, flags=CHECK_ROOT | CHECK_PROOFS, key=0, expect=r33)                        # a payload byte: root first
    add(ROOT, body, fill={1, 2}, flags=CHECK_ROOT, key=0, expect=r33)                          # ... and nothing is filled
    add(PROOF, body, flags=CHECK_PROOFS, key=0)
    bad_root = fm.outcome(body)[1]
    msg = o.verify(bad_root, body[0][:64], keys[0].tobytes(), 0)
    add(msg, body, key=0)                                                                      # ... with a key alone
    add(0, body)
    wrong = o.verify(r33, s33[0][:64], keys[1].tobytes(), 0)
    add(wrong, s33, flags=CHECK_ROOT | CHECK_PROOFS, key=1, expect=r33)                        # a wrong leader
    add(wrong, _blank(s33, [4, 30]), fill={4, 30}, flags=CHECK_PROOFS, key=1)                  # ... fills all the same
    add(0, s9, flags=CHECK_PROOFS, key=1)
    b.finish()
    assert msg != 0 and wrong != 0 and bad_root != r33
    eng = _engine(64, payload=len(b.member) * 1232, fec=(len(b.desc), len(b.member)), keys=2)
    try:
        codes, _ = _all_forms(eng, b, keys, "codes")
        assert codes.tolist() == [want[i] for i in range(len(codes))], codes.tolist()
    finally:
        eng.close()


def test_root_proof_and_signature_codes():
    """A wrong expect; one flipped proof byte in a non-FILL member, ignored when that member is FILL or CHECK_PROOFS
    is clear; a flipped payload byte under CHECK_ROOT, under CHECK_PROOFS and under a key alone; a wrong leader, whose
    set is filled all the same"""
    _other_codes()


@_once
def _bad_descriptors():
    keys = np.frombuffer(ks._key(0)[0] + ks._key(1)[0], np.uint8).reshape(2, 32)
    s9, s5 = _signed(_size(9), 0), _signed(_size(5), 1)
    b = _Batch(26)
    good = []

    def ok():
        """a good set whose member 1 lacks its proof and has FILL"""
        t = len(good) % 2
        good.append(b.add(_blank(s9 if t else s5, [1]), fill={1}, flags=CHECK_PROOFS, key=t ^ 1))

    ok()
    first = b.members[0][0]
    for row, members in (((0, 0, NO_SIG, 0, 0), ()),                           # no leaf
                         ((0, 257, NO_SIG, 0, 0), ()),                         # more than 256
                         ((0, 0xFFFF, NO_SIG, 0, 0), ()),
                         ((0xFFFFFFFF, 1, NO_SIG, 0, 0), ()),                  # the member range, no wrap
                         ((0xFFFFFFFF, 256, NO_SIG, 0, 0), ()),
                         ((0, 5, 2, 0, 0), ()),                                # a key past the keys
                         ((0, 5, 0xFFFE, 0, 0), ()),
                         ((None, 1, NO_SIG, 0, 0), ((0xFFFFFFFF, 0),)),        # a member past the arena, no wrap
                         ((None, 2, NO_SIG, 0, 0), ((first, 0), (0xFFFFF000, FILL)))):
        b.raw(row, DESC, members)
        ok()
    # a code shred cut short ends the arena, behind five more good sets: members around the two bounds
    for _ in range(5):
        ok()
    at = b.ar.put(s9[8][:1210], 3)
    A = len(b.ar.b)
    assert at + 1203 <= A < at + 1228
    # (the third: 1203 bytes fit and are looked at; whatever lies there is no one-leaf set, or a code shred out of range)
    junk = bytes(b.ar.b[A - 1203:]) + bytes(25)
    assert fm.member_error([junk])
    late = [b.raw((None, 1, NO_SIG, 0, 0), DESC, [(A - 1202, 0)]),             # 1203 bytes do not fit
            b.raw((None, 1, NO_SIG, 0, 0), DESC, [(at, FILL)]),                # 1203 fit, a code shred's 1228 do not
            b.raw((None, 1, NO_SIG, 0, 0), DESC if junk[0x40] & 0xf0 in sm.CODE_TYPES else MEMBER, [(A - 1203, 0)]),
            b.raw((None, 1, NO_SIG, 0, 0), DESC, [(A, 0)]),
            b.raw((len(b.members), 1, NO_SIG, 0, 0), DESC)]                  # member0 + cnt one past member_cnt
    # each of them between two of the good sets
    order = list(range(late[0] - 5))
    for t in range(5):
        order += [late[t], late[0] - 5 + t]
    b.rows, b.sets = [b.rows[i] for i in order], [b.sets[i] for i in order]
    good = [order.index(i) for i in good]
    b.finish(last_flush=True)
    assert b.A == A and int(b.desc["member0"][-2]) == len(b.member) and len(order) == len(set(order)) == 29
    eng = _engine(64, payload=len(b.member) * 1232, fec=(len(b.desc), len(b.member)), keys=2)
    try:
        codes, roots = _all_forms(eng, b, keys, "bad descriptors")
        assert all(codes[i] == 0 for i in good) and (codes == DESC).sum() >= 13 and len(good) == 15
        # the device form alone sees the caller's slots: one past the slots is bad
        d, nsig = _number(b.desc)
        d["sig_idx"][good[2]] = nsig
        want, wroot, after = b.want(keys)
        got, root, bytes_after = _device(eng, b, keys, d, nsig)
        wroot = wroot.copy()
        want[good[2]] = DESC
        wroot[good[2]] = 0
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(root, wroot)
        # that set's FILL member stays blank; every other byte is as before
        st = b.sets[good[2]]
        lo = GUARD + st["offs"][1] + fm.moff(st["shreds"][1])
        hi = lo + 20 * fm.depth(len(st["shreds"]))
        after[lo:hi] = 0
        assert bytes_after.tobytes() == after.tobytes()
    finally:
        eng.close()


def test_bad_descriptors_between_good_sets():
    """Bad sets, each between two good ones that keep their codes, roots and bytes: cnt 0 and above 256, the member
    range, the key, the slot (device form), members past the arena by the data and the code bound"""
    _bad_descriptors()


# ---- 5: signatures ------------------------------------------------------------------------------------------

@_once
def _signatures():
    g = trees()
    i17 = _size(17)
    keys = np.frombuffer(ks._key(0)[0] + ks._key(1)[0], np.uint8).reshape(2, 32)
    # sig_cnt = 0: roots only, no verify kernel; d_root NULL
    b = _Batch(27)
    for n in (1, 5, 17, 64):
        b.add(built_set(_size(n)), flags=CHECK_PROOFS)
    b.finish()
    eng = _engine(64, payload=len(b.member) * 1232, fec=(32, 2048), keys=2)
    try:
        codes, roots = _all_forms(eng, b, (), "no signatures")
        assert not codes.any()
        np.testing.assert_array_equal(roots, g["root"][[_size(n) for n in (1, 5, 17, 64)]])
        for f in (_device, _registered, _plain):
            got, root, _ = f(eng, b, (), want_root=False)
            assert not got.any() and root is None
        # set by set the same as the per-shred call on the same shreds: every shred's root is its set's, and the keyed
        # shred's code the set's
        b2 = _Batch(28)
        b2.add(_signed(i17, 0), flags=CHECK_PROOFS, key=0)
        b2.add([x[:40] + bytes([x[40] ^ 4]) + x[41:] for x in _signed(i17, 1)], flags=CHECK_PROOFS, key=1)   # S, in every member
        s3 = _signed(_size(33), 1)
        b2.add(s3, flags=CHECK_PROOFS, key=0)                                    # the other leader
        b2.finish()
        set_codes, set_roots = _all_forms(eng, b2, keys, "against the per-shred call")
        assert set_codes[0] == 0 and set_codes[1] != 0 and set_codes[2] != 0
        import torch
        eng.shreds_prepare(len(b2.member), 2)
        sd = np.zeros(len(b2.member), engine.SHRED_DESC_DTYPE)
        sd["off"] = b2.member["off"]
        sd["sz"] = [len(s) for st in b2.sets for s in st["shreds"]]
        sd["key_idx"] = NO_SIG
        sd["flags"] = engine.FDGPU_SHRED_STRICT_LEAF
        firsts = b2.desc["member0"]
        sd["key_idx"][firsts] = b2.desc["key_idx"]
        sd["sig_idx"][firsts] = np.arange(3)
        raw, o = b2.guarded()
        a = torch.from_numpy(raw[o:o + b2.A + SLACK].copy()).cuda()
        dd = torch.from_numpy(sd.view(np.uint8)).cuda()
        kk = torch.from_numpy(keys.reshape(-1).copy()).cuda()
        out = torch.full((len(sd),), 7, dtype=torch.int8, device="cuda")
        root = torch.zeros((len(sd), 32), dtype=torch.uint8, device="cuda")
        eng.verify_shreds_device(a.data_ptr(), b2.A, dd.data_ptr(), len(sd), 3, kk.data_ptr(), 2, out.data_ptr(), root.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out, root = out.cpu().numpy(), root.cpu().numpy()
        for t in range(3):
            lo, n = int(firsts[t]), int(b2.desc["cnt"][t])
            assert (root[lo:lo + n] == set_roots[t]).all() and out[lo] == set_codes[t] and not out[lo + 1:lo + n].any()
    finally:
        eng.close()
    # a pinned leader over 20 sets on the throughput path
    b3 = _Batch(29)
    for t in range(20):
        b3.add(fm.build_set(3, 2, t % 3, 300 + t, lambda r: ks._sign(0, r)[0]), flags=CHECK_PROOFS, key=0)
    for t in range(6):
        b3.add(fm.build_set(2, 2, t % 3, 400 + t, lambda r: ks._sign(10 + t, r)[0]), flags=CHECK_PROOFS, key=1 + t)
    b3.finish()
    keys3 = np.frombuffer(ks._key(0)[0] + b"".join(ks._key(10 + t)[0] for t in range(6)), np.uint8).reshape(7, 32)
    eng = _engine(4096, fec=(26, len(b3.member)), keys=7, half=1, small_batch_max=0)
    try:
        eng.set_pinned_keys([ks._key(0)[0]])
        got, _, _ = _device(eng, b3, keys3)
        assert not got.any()
        assert eng.pinned_count() == (1, 20), eng.pinned_count()
    finally:
        eng.close()


def test_signatures():
    """sig_cnt = 0; no roots asked for; agreement with verify_shreds_device on the same shreds, set by set; a pinned
    leader over 20 sets gives pinned_count = (1, 20)"""
    _signatures()


# ---- 6: refusals and chunks ---------------------------------------------------------------------------------

@_once
def _refusals():
    import torch
    keys = np.frombuffer(ks._key(0)[0], np.uint8).reshape(1, 32)
    keys3 = np.concatenate([keys, keys, keys])
    g = trees()
    b = _Batch(30)
    for t in range(6):
        b.add(_signed(_size((33, 9, 17)[t % 3]), 0), flags=CHECK_PROOFS, key=0)
    b.finish()
    zero = np.zeros(6, np.int8)
    roots = g["root"][[_size((33, 9, 17)[t % 3]) for t in range(6)]]
    nm = len(b.member)
    assert nm == 118
    eng = _engine(4, payload=40 * 1232)
    try:
        # unprepared
        assert _refused(_device, eng, b, keys) == -3
        assert _refused(_registered, eng, b, keys) == -3
        assert _refused(_plain, eng, b, keys) == -3
        for bad in ((0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 0x10000), (1 << 31, 10, 1), (1, 1 << 31, 1)):
            assert _refused(eng.fec_prepare, *bad) == -1, bad
        eng.fec_prepare(6, nm, 2)
        # six sets fit, six signatures do not: the context has four slots
        assert _refused(_device, eng, b, keys) == -1
        d, nsig = _number(b.desc)
        d4 = d.copy()
        d4["key_idx"][4:] = NO_SIG
        got, root, _ = _device(eng, b, keys, d4, 4)
        np.testing.assert_array_equal(got, zero)
        np.testing.assert_array_equal(root, roots)
        assert _refused(_device, eng, b, keys3, d4, 4) == -1                    # 3 keys, 2 prepared
        assert _refused(_registered, eng, b, keys3) == -1
        both = _Batch(30)
        for s in b.sets + b.sets:
            both.add(s["shreds"], flags=CHECK_PROOFS, key=0)
        both.finish()
        db = both.desc.copy()
        db["key_idx"] = NO_SIG
        assert _refused(_device, eng, both, keys, db, 0) == -1                   # 12 sets, 236 members
        db6 = _Batch(30)
        db6.rows, db6.members, db6.sets = both.rows[:6], both.members, both.sets[:6]
        db6.ar = both.ar
        db6.b, db6.A = both.b, both.A
        db6.desc, db6.member = db[:6].copy(), both.member
        assert _refused(_device, eng, db6, keys, db6.desc, 0) == -1              # 6 sets, 236 members
        # misaligned keys, roots and expected roots
        raw, o = b.guarded()
        a = torch.from_numpy(raw[o:o + b.A + SLACK].copy()).cuda()
        dd = torch.from_numpy(d4.view(np.uint8)).cuda()
        mm = torch.from_numpy(b.member.view(np.uint8).copy()).cuda()
        kk = torch.zeros(64 + 16, dtype=torch.uint8, device="cuda")
        out = torch.zeros(6, dtype=torch.int8, device="cuda")
        rr = torch.zeros(6 * 32 + 16, dtype=torch.uint8, device="cuda")
        ee = torch.zeros(6 * 32 + 16, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def call(k_off, r_off, e_off):
            eng.verify_fec_sets_device(a.data_ptr(), b.A, dd.data_ptr(), 6, mm.data_ptr(), nm, 4, kk.data_ptr() + k_off, 1,
                                       ee.data_ptr() + e_off, out.data_ptr(), rr.data_ptr() + r_off, st)

        assert _refused(call, 8, 0, 0) == -1 and _refused(call, 0, 4, 0) == -1 and _refused(call, 0, 0, 1) == -1
        call(16, 16, 16)
        torch.cuda.synchronize()
        # the host form cuts chunks on set boundaries instead: 12 sets through 6 sets, 118 members, 4 slots and a
        # staging slot of 40 shreds (33 + 9 would not fit: the first chunk is one set)
        for f in (_registered, _plain):
            got, root, _ = f(eng, both, keys)
            np.testing.assert_array_equal(got, np.concatenate([zero, zero]))
            np.testing.assert_array_equal(root, np.concatenate([roots, roots]))
        # CHECK_ROOT without expect; a set that no chunk holds
        c = _Batch(31)
        c.add(_signed(_size(9), 0), flags=CHECK_ROOT)
        c.finish()
        assert _refused(_registered, eng, c, keys) == -1 and _refused(_plain, eng, c, keys) == -1
        big = _Batch(32)
        big.add(_signed(_size(64), 0), key=0)
        big.add(_signed(_size(129), 0), key=0)
        big.finish()
        assert _refused(_plain, eng, big, keys) == -1                            # 64 members, the staging slot holds 40
        assert _refused(_registered, eng, big, keys) == -1                       # 129 members, 118 prepared
        # a smaller size changes nothing, a larger one reallocates
        eng.fec_prepare(1, 1, 1)
        np.testing.assert_array_equal(_device(eng, b, keys, d4, 4)[0], zero)
        eng.fec_prepare(12, 2 * nm, 3)
        np.testing.assert_array_equal(_device(eng, both, keys3, db, 0)[0], np.concatenate([zero, zero]))
        got, root, _ = _registered(eng, big, keys)
        assert not got.any()
        # the async pipeline holds a transaction: the synchronous calls' refusal
        sig, pub = ks._sign(0, b"x" * 40)
        assert eng.submit(sig + pub + b"x" * 40, 0, 64, 96, 1, 7) == 0
        assert _refused(_registered, eng, b, keys) == -1
        assert _refused(_plain, eng, b, keys) == -1
        eng.flush()
        tags, codes = eng.poll(blocking=True)
        assert list(tags) == [7] and list(codes) == [0]
        np.testing.assert_array_equal(_plain(eng, b, keys)[0], zero)
        # a faulted context
        eng.debug_fault()
        assert _refused(_device, eng, b, keys, d4, 4) == -3
        assert _refused(_plain, eng, b, keys) == -3
        assert _refused(eng.fec_prepare, 100, 1000, 1) == -3
    finally:
        eng.close()
    # no staging: the device form and a registered arena work, any other memory is refused
    eng = _engine(16, fec=(6, nm), keys=1)
    try:
        np.testing.assert_array_equal(_device(eng, b, keys)[0], zero)
        np.testing.assert_array_equal(_registered(eng, b, keys)[0], zero)
        assert _refused(_plain, eng, b, keys) == -3
    finally:
        eng.close()


def test_refusals_and_chunks():
    _refusals()
