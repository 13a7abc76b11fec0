"""CPU: Merkle shred descriptors (fdgpu_shred_desc_t).  The struct's layout in the header and in the numpy
dtype; the constants; the new entry points' place in the header and the bindings; the rules of
firedancer_amd/csrc/fd_shred_desc.h, driven by the stand-alone program fd_shred_desc_check.c that build.py builds;
and tests/shred_model.py against every result the reference recorded in tests/golden/shreds.npz."""
import os
import re
import subprocess

import numpy as np

from firedancer_amd import build, engine
from tests import shred_model as sm
from tests.test_abi_layout import _c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["off", "sz", "key_idx", "sig_idx", "flags"]


def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "shreds.npz")))


def case_bytes(g, i, width=1228 + 7):
    """case i's shred with its patch applied, zero-padded to width bytes"""
    b = bytearray(g["shreds"][g["c_base"][i]].tobytes().ljust(width, b"\0"))
    b[1228:] = bytes(width - 1228)
    o, n = int(g["c_off"][i]), int(g["c_len"][i])
    b[o:o + n] = g["c_bytes"][i, :n].tobytes()
    return bytes(b)


def expected(g, i, sem):
    """(code, root) the reference gives case i: the parse, then fd_shred_merkle_root, then the verify"""
    variant = case_bytes(g, i)[0x40] if g["c_sz"][i] > 0x40 else 0
    if not g["c_parse"][i] or variant in (0xa5, 0x5a):
        return sm.ERR_PARSE, bytes(32)
    if not g["c_merkle"][i]:
        return sm.ERR_MERKLE, bytes(32)
    return int(g["c_code"][sem, i]), g["c_root"][i].tobytes()


def test_shred_desc_layout_matches_c():
    dt = engine.SHRED_DESC_DTYPE
    assert list(dt.names) == FIELDS
    size, offs = _c_layout([("fdgpu_shred_desc_t", FIELDS)])["fdgpu_shred_desc_t"]
    assert size == 16 and dt.itemsize == 16
    assert [offs[f] for f in FIELDS] == [0, 4, 6, 8, 12]
    assert [dt.fields[f][1] for f in FIELDS] == [0, 4, 6, 8, 12]
    assert [dt.fields[f][0] for f in FIELDS] == ["<u4", "<u2", "<u2", "<u4", "<u4"]


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "fd_ed25519_gpu.h")).read()
    hdr = open(os.path.join(build.CSRC, "fd_shred_desc.h")).read()

    def num(text, name):
        return int(re.search(r"#define\s+%s\s+\((-?\w+?)[uU]?\)" % name, text).group(1), 0)

    assert num(txt, "FDGPU_ERR_SHRED_PARSE") == engine.FDGPU_ERR_SHRED_PARSE == num(hdr, "FD_SHRED_ERR_PARSE") == sm.ERR_PARSE == -19
    assert num(txt, "FDGPU_ERR_SHRED_MERKLE") == engine.FDGPU_ERR_SHRED_MERKLE == num(hdr, "FD_SHRED_ERR_MERKLE") == sm.ERR_MERKLE == -20
    assert num(txt, "FDGPU_ERR_DESC") == num(hdr, "FD_SHRED_ERR_DESC") == sm.ERR_DESC == engine.FDGPU_ERR_DESC == -18
    assert num(txt, "FDGPU_SHRED_NO_SIG") == engine.FDGPU_SHRED_NO_SIG == num(hdr, "FD_SHRED_NO_SIG") == sm.NO_SIG == 0xFFFF
    assert num(txt, "FDGPU_SHRED_STRICT_LEAF") == engine.FDGPU_SHRED_STRICT_LEAF == num(hdr, "FD_SHRED_STRICT_LEAF") == sm.STRICT_LEAF == 1
    assert "fd_shred_desc.h" in build.HIP_DEPS and "fd_gpu_sha256.h" in build.HIP_DEPS


def test_shred_entry_points_are_declared_and_bound():
    names = ("fdgpu_ed25519_shreds_prepare", "fdgpu_ed25519_verify_shreds_device", "fdgpu_ed25519_verify_shreds_host",
             "fdgpu_sha256_batch_device", "fdgpu_sha256_batch_host")
    txt = open(os.path.join(ROOT, "include", "fd_ed25519_gpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = engine.load_library()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in engine.EXPORTS, n
        assert hasattr(lib, n), n
    for m in ("shreds_prepare", "verify_shreds_host", "verify_shreds_device"):
        assert callable(getattr(engine.Engine, m))
    assert callable(engine.sha256_batch_host) and callable(engine.sha256_batch_device)


def test_shred_desc_check_program():
    exe = build.build_shred_desc_check()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_fixture_is_what_the_generator_promises():
    g = fixture()
    n = len(g["c_base"])
    assert g["shreds"].shape == (186, 1228) and n >= 186 + 300 and g["keys"].shape == (5, 32)
    assert (g["c_len"][:186] == 0).all() and (g["c_base"][:186] == np.arange(186)).all()
    assert (g["c_sz"][:186] == g["shred_sz"]).all() and (g["c_key"][:186] == g["shred_key"]).all()
    # every original parses, has a root and verifies in both semantics
    assert g["c_parse"][:186].all() and g["c_merkle"][:186].all() and not g["c_code"][:, :186].any()
    assert sorted(set(g["shreds"][:, 0x40].tolist())) == [0x65, 0x66, 0x76, 0x95, 0x96, 0xb6]
    assert len({g["shreds"][i, :64].tobytes() for i in range(186)}) == 5
    # the mutants reach every outcome
    m = slice(186, n)
    assert (g["c_parse"][m] == 0).sum() > 50 and ((g["c_parse"][m] == 1) & (g["c_merkle"][m] == 0)).sum() > 20
    for sem in (0, 1):
        assert set(g["c_code"][sem, m][g["c_merkle"][m] == 1].tolist()) == {0, -1, -2, -3}


def test_model_reproduces_the_reference():
    """Every root and every outcome short of the signature: the model against the reference's recorded results"""
    g = fixture()
    for i in range(len(g["c_base"])):
        code, root = sm.outcome(case_bytes(g, i), int(g["c_sz"][i]))
        want, want_root = expected(g, i, 0)
        if want in (sm.ERR_PARSE, sm.ERR_MERKLE):
            assert code == want and root is None, (i, code, want)
        else:
            assert code == 0 and root == want_root, (i, code, want)


def test_model_strict_leaf_is_the_resolvers_rule():
    """fd_fec_resolver.c:412 on top of eqvoc's outcome: a leaf index at or past 2^depth, and nothing else"""
    g = fixture()
    changed = 0
    for i in range(len(g["c_base"])):
        b, sz = case_bytes(g, i), int(g["c_sz"][i])
        code, root = sm.outcome(b, sz)
        scode, sroot = sm.outcome(b, sz, sm.STRICT_LEAF)
        if code:
            assert (scode, sroot) == (code, root)
            continue
        t, d = b[0x40] & 0xf0, b[0x40] & 0xf
        idx, fec = int.from_bytes(b[0x49:0x4d], "little"), int.from_bytes(b[0x4f:0x53], "little")
        leaf = idx - fec if t in sm.DATA_TYPES else int.from_bytes(b[0x57:0x59], "little") + int.from_bytes(b[0x53:0x55], "little")
        if leaf >= (1 << d):
            assert (scode, sroot) == (sm.ERR_MERKLE, None), i
            changed += 1
        else:
            assert (scode, sroot) == (0, root), i
    assert changed >= 6
