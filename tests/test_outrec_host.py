"""The output buffers' content-record table (g-vom_amd/csrc/gvom_outrec.h: which output buffer has which bitmap, and when a bitmap
must restart) checked on the CPU: tests/outrec_host_test.cpp, a program with its own main, is compiled with AddressSanitizer and
UndefinedBehaviorSanitizer and run -- insert, re-use, forget, size change, eviction, destroy.  No GPU and nothing loaded into
Python: the table is plain host code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_table_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "outrec_host_test")
    src = os.path.join(ROOT, "tests", "outrec_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "outrec host test ok" in run.stdout
