"""CPU: per-signature descriptors (fdgpu_sig_desc_t).  The struct's layout in the header and in the numpy
dtype; the validity test, packed size and placement of firedancer_amd/csrc/fd_sig_desc.h, driven by the stand-alone
program fd_sig_desc_check.c; and the new entry points' place in the header and the bindings."""
import os
import re
import subprocess

from firedancer_amd import build, engine
from tests.test_abi_layout import _c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sig_desc_layout_matches_c():
    dt = engine.SIG_DESC_DTYPE
    fields = ["sig_off", "pub_off", "msg_off", "msg_sz"]
    assert list(dt.names) == fields
    size, offs = _c_layout([("fdgpu_sig_desc_t", fields)])["fdgpu_sig_desc_t"]
    assert size == 16 and dt.itemsize == 16
    assert [offs[f] for f in fields] == [0, 4, 8, 12]
    assert [dt.fields[f][1] for f in fields] == [0, 4, 8, 12]
    assert all(dt.fields[f][0] == "<u4" for f in fields)


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "fd_ed25519_gpu.h")).read()
    assert int(re.search(r"#define\s+FDGPU_ERR_DESC\s+\((-?\d+)\)", txt).group(1)) == engine.FDGPU_ERR_DESC == -18
    assert int(re.search(r"#define\s+FDGPU_MSG_MAX\s+\((\d+)UL\)", txt).group(1)) == engine.FDGPU_MSG_MAX == 65439
    hdr = open(os.path.join(build.CSRC, "fd_sig_desc.h")).read()
    assert int(re.search(r"#define\s+FD_SIG_DESC_MSG_MAX\s+\((\d+)UL\)", hdr).group(1)) == engine.FDGPU_MSG_MAX


def test_sig_desc_check_program(tmp_path):
    exe = str(tmp_path / "fd_sig_desc_check")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(build.CSRC, "fd_sig_desc_check.c")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_sigs_entry_points_are_declared_and_bound():
    names = ("fdgpu_ed25519_sigs_prepare", "fdgpu_ed25519_verify_sigs_device", "fdgpu_ed25519_verify_sigs_host")
    txt = open(os.path.join(ROOT, "include", "fd_ed25519_gpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = engine.load_library()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in engine.EXPORTS, n
        assert hasattr(lib, n), n
    for m in ("sigs_prepare", "verify_sigs_host", "verify_sigs_device"):
        assert callable(getattr(engine.Engine, m))
