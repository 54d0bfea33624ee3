"""The device sets' layout table (g-vom_amd/csrc/gvom_setlayout.h: how large the allocation of a map set or of a product is, and
where each of its parts lies) checked on the CPU: tests/setlayout_host_test.cpp, a program with its own main, is compiled with
AddressSanitizer and UndefinedBehaviorSanitizer and run -- every kind at small, odd and the largest shapes: parts inside the
allocation, aligned, disjoint, as long as their shapes say, and unknown parts refused.  No GPU and nothing loaded into Python: the
table is plain host code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_layouts_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "setlayout_host_test")
    src = os.path.join(ROOT, "tests", "setlayout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "setlayout host test ok" in run.stdout
