"""CPU: the host side of fdgpu_ed25519_set_pinned_keys' key list (firedancer_amd/csrc/fd_pin_list.h: the cap, the
de-duplication that gives every listed key its slot), driven by the stand-alone program fd_pin_list_check.c, and the
new entry points' place in the header and the bindings."""
import os
import re
import subprocess

from firedancer_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pin_list_check_program(tmp_path):
    exe = str(tmp_path / "fd_pin_list_check")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(build.CSRC, "fd_pin_list_check.c")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_pin_entry_points_are_declared_and_bound():
    names = ("fdgpu_ed25519_set_pinned_keys", "fdgpu_ed25519_pin_cap", "fdgpu_ed25519_pinned_count")
    txt = open(os.path.join(ROOT, "include", "fd_ed25519_gpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in engine.EXPORTS, n
    for m in ("set_pinned_keys", "pin_cap", "pinned_count"):
        assert callable(getattr(engine.Engine, m))
