"""CPU: the host decisions of device memory and table placement (libfm_amd/csrc/fmx_place_plan.h: layout, pool bound, prefix rule, class
book, mapping order, the arena's sequence and the owner of a chunked range) against their specification and a fake device with every
call of the virtual-memory API failing in turn -- scripts/place_plan_check.cpp, compiled here with the host compiler (no sanitizer:
that run is done by hand, see the program's head)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_place_plan_check(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "place_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "scripts", "place_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("place_plan_check: ok")
