"""CPU: FEC sets (fdgpu_fec_desc_t / fdgpu_fec_member_t).  The structs' layout in the header and in the
numpy dtypes; the constants; the entry points' place in the header and the bindings; the rules of
firedancer_amd/csrc/fd_fec_desc.h, driven by the stand-alone program fd_fec_desc_check.c that build.py builds; and
tests/fec_model.py against every tree the reference recorded in tests/golden/fec_trees.npz and against the real sets
of tests/golden/shreds.npz."""
import functools
import os
import re
import subprocess

import numpy as np

from firedancer_amd import build, engine
from tests import fec_model as fm
from tests import shred_model as sm
from tests.test_abi_layout import _c_layout
from tests.test_shred_desc import fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC_FIELDS = ["member0", "cnt", "key_idx", "sig_idx", "flags"]
MEMBER_FIELDS = ["off", "flags"]


@functools.lru_cache(maxsize=None)
def trees():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "fec_trees.npz")))


@functools.lru_cache(maxsize=None)
def built_set(i, sign=None):
    """set i of fec_trees.npz rebuilt from its recorded seed (unsigned unless sign is given), held against the
    recorded leaf hashes: a builder that drifts fails here"""
    g = trees()
    shreds = fm.build_set(int(g["data_cnt"][i]), int(g["code_cnt"][i]), int(g["cls"][i]), int(g["seed"][i]),
                          sign or (lambda r: bytes(64)))
    f, n = int(g["first"][i]), int(g["n"][i])
    assert len(shreds) == n
    assert b"".join(fm.leaf_hash(s) for s in shreds) == g["leaves"][f:f + n].tobytes(), i
    return shreds


@functools.lru_cache(maxsize=None)
def real_sets():
    """[(shreds in tree order, root, leader key index)]: the complete sets of shreds.npz, grouped by their signature"""
    g = fixture()
    by_sig = {}
    for i in range(186):
        s = g["shreds"][i, :g["shred_sz"][i]].tobytes()
        by_sig.setdefault(s[:64], []).append((i, s))
    out = []
    for group in by_sig.values():
        def leaf(s):
            slot, idx, ver, fec, a, b, c = fm._fields(s)
            return idx - fec if s[0x40] & 0xf0 in sm.DATA_TYPES else c + a
        group = sorted(group, key=lambda e: leaf(e[1]))
        assert [leaf(s) for _, s in group] == list(range(len(group)))
        i0 = group[0][0]
        out.append(([s for _, s in group], g["c_root"][i0].tobytes(), int(g["shred_key"][i0])))
    return out


def test_layouts_match_c():
    dt, mt = engine.FEC_DESC_DTYPE, engine.FEC_MEMBER_DTYPE
    lay = _c_layout([("fdgpu_fec_desc_t", DESC_FIELDS), ("fdgpu_fec_member_t", MEMBER_FIELDS)])
    size, offs = lay["fdgpu_fec_desc_t"]
    assert size == 16 and dt.itemsize == 16 and list(dt.names) == DESC_FIELDS
    assert [offs[f] for f in DESC_FIELDS] == [dt.fields[f][1] for f in DESC_FIELDS] == [0, 4, 6, 8, 12]
    assert [dt.fields[f][0] for f in DESC_FIELDS] == ["<u4", "<u2", "<u2", "<u4", "<u4"]
    size, offs = lay["fdgpu_fec_member_t"]
    assert size == 8 and mt.itemsize == 8 and list(mt.names) == MEMBER_FIELDS
    assert [offs[f] for f in MEMBER_FIELDS] == [mt.fields[f][1] for f in MEMBER_FIELDS] == [0, 4]


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "fd_ed25519_gpu.h")).read()
    hdr = open(os.path.join(build.CSRC, "fd_fec_desc.h")).read()

    def num(text, name):
        return int(re.search(r"#define\s+%s\s+\((-?\w+?)[uU]?\)" % name, text).group(1), 0)

    assert num(txt, "FDGPU_ERR_FEC_MEMBER") == engine.FDGPU_ERR_FEC_MEMBER == num(hdr, "FD_FEC_ERR_MEMBER") == fm.ERR_MEMBER == -21
    assert num(txt, "FDGPU_ERR_FEC_ROOT") == engine.FDGPU_ERR_FEC_ROOT == num(hdr, "FD_FEC_ERR_ROOT") == fm.ERR_ROOT == -22
    assert num(txt, "FDGPU_ERR_FEC_PROOF") == engine.FDGPU_ERR_FEC_PROOF == num(hdr, "FD_FEC_ERR_PROOF") == fm.ERR_PROOF == -23
    assert num(txt, "FDGPU_FEC_LEAF_MAX") == engine.FDGPU_FEC_LEAF_MAX == num(hdr, "FD_FEC_LEAF_MAX") == fm.LEAF_MAX == 256
    assert num(txt, "FDGPU_FEC_FILL") == engine.FDGPU_FEC_FILL == num(hdr, "FD_FEC_FILL") == fm.FILL == 1
    assert num(txt, "FDGPU_FEC_CHECK_ROOT") == engine.FDGPU_FEC_CHECK_ROOT == num(hdr, "FD_FEC_CHECK_ROOT") == fm.CHECK_ROOT == 1
    assert num(txt, "FDGPU_FEC_CHECK_PROOFS") == engine.FDGPU_FEC_CHECK_PROOFS == num(hdr, "FD_FEC_CHECK_PROOFS") == fm.CHECK_PROOFS == 2
    assert fm.ERR_DESC == engine.FDGPU_ERR_DESC
    assert "fd_fec_desc.h" in build.HIP_DEPS


def test_entry_points_are_declared_and_bound():
    names = ("fdgpu_ed25519_fec_prepare", "fdgpu_ed25519_verify_fec_sets_device", "fdgpu_ed25519_verify_fec_sets_host")
    txt = open(os.path.join(ROOT, "include", "fd_ed25519_gpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = engine.load_library()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in engine.EXPORTS, n
        assert hasattr(lib, n), n
    for m in ("fec_prepare", "verify_fec_sets_host", "verify_fec_sets_device"):
        assert callable(getattr(engine.Engine, m))


def test_fec_desc_check_program():
    exe = build.build_fec_desc_check()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_fixture_is_what_the_generator_promises():
    g = trees()
    assert tuple(g["n"].tolist()) == fm.SIZES
    assert (g["data_cnt"].astype(int) + g["code_cnt"] == g["n"]).all() and (g["data_cnt"] >= 1).all()
    assert (g["code_cnt"][1:] >= 1).all() and set(g["cls"].tolist()) == {0, 1, 2}
    assert g["leaves"].shape == (int(g["n"].sum()), 32) and g["proofs"].shape == (int(g["n"].sum()), 160)
    assert [fm.depth(int(n)) for n in g["n"]] == g["depth"].tolist()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fec_trees.npz")) < (1 << 20)


def test_model_reproduces_the_reference_trees():
    """every recorded leaf, root and proof, the odd layers of 3, 5, 7, 9, 17, 31, 33, 63, 65, 67, 127, 129, 134 and 255
    among them"""
    g = trees()
    for i, n in enumerate(g["n"].tolist()):
        shreds = built_set(i)
        f, D = int(g["first"][i]), int(g["depth"][i])
        root, layers = fm.tree([fm.leaf_hash(s) for s in shreds])
        assert root == g["root"][i].tobytes(), n
        assert len(layers) == D + 1 and [len(x) for x in layers] == [(n + (1 << l) - 1) >> l for l in range(D + 1)]
        for j in range(n):
            assert fm.proof(layers, j) == g["proofs"][f + j, :20 * D].tobytes(), (n, j)
            assert not g["proofs"][f + j, 20 * D:].any()
        # the builder wrote these proofs into the shreds, so the set passes every check
        assert fm.outcome(shreds, flags=fm.CHECK_ROOT | fm.CHECK_PROOFS, expect=root) == \
            (0, root, [g["proofs"][f + j, :20 * D].tobytes() for j in range(n)])


def test_model_reproduces_the_real_sets():
    """the five complete sets of the reference's archives (25, 33, 41 and 23 chained, 64 resigned): the rebuilt root is
    the recorded one, and every proof byte the shreds carry is the tree's"""
    sets = real_sets()
    assert sorted(len(s) for s, _, _ in sets) == [23, 25, 33, 41, 64]
    for shreds, root, _ in sets:
        code, got, proofs = fm.outcome(shreds, flags=fm.CHECK_ROOT | fm.CHECK_PROOFS, expect=root)
        assert code == 0 and got == root, len(shreds)
        for j, s in enumerate(shreds):
            m = fm.moff(s)
            assert s[m:m + 20 * fm.depth(len(shreds))] == proofs[j]


def test_model_refuses_what_the_rules_name():
    """one mutation per rule in the middle member of the real set of 33, and the two flags"""
    shreds, root, _ = next(e for e in real_sets() if len(e[0]) == 33)
    assert fm.outcome(shreds, flags=3, expect=root)[0] == 0

    def mutated(j, off, new):
        out = list(shreds)
        b = bytearray(out[j])
        b[off:off + len(new)] = new
        out[j] = bytes(b)
        return out

    m = fm.moff(shreds[5])
    for off, new in ((0x41, b"\x01"), (0x4d, bytes([shreds[5][0x4d] ^ 1])), (0x4e, bytes([shreds[5][0x4e] ^ 0x80])), (0x4f, b"\x06"), (0x40, bytes([0x86])), (0x40, bytes([0x95])),
                     (0x53, b"\x07"), (m - 32, b"\x00\x01"), (3, bytes([shreds[5][3] ^ 1]))):
        assert fm.outcome(mutated(5, off, new))[0] == fm.ERR_MEMBER, off
    assert fm.outcome(mutated(20, 0x53, b"\x0b"))[0] == fm.ERR_MEMBER          # a code member's data_cnt
    assert fm.outcome(shreds[:32])[0] == fm.ERR_MEMBER                          # data_cnt + code_cnt is not cnt
    assert fm.outcome(shreds[1:])[0] == fm.ERR_MEMBER                           # positions
    bad = mutated(5, m + 3, bytes([shreds[5][m + 3] ^ 1]))
    assert fm.outcome(bad, flags=fm.CHECK_PROOFS)[0] == fm.ERR_PROOF
    assert fm.outcome(bad, flags=fm.CHECK_PROOFS, fill={5})[0] == 0 and fm.outcome(bad)[0] == 0
    assert fm.outcome(shreds, flags=fm.CHECK_ROOT, expect=bytes(32))[0] == fm.ERR_ROOT
    body = mutated(5, 200, bytes([shreds[5][200] ^ 1]))
    assert fm.outcome(body, flags=fm.CHECK_ROOT, expect=root)[0] == fm.ERR_ROOT
    assert fm.outcome(body, flags=fm.CHECK_PROOFS)[0] == fm.ERR_PROOF
