"""Memory safety of the host side of the preview-stream JPEG encoder (header builder, bound, argument checks,
csrc/jpeg_tables.hpp): tests/native/jpeg_host_check.cpp is built as a stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a process of its own.  Nothing loaded into python runs under a sanitizer."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_host_parts_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "jpeg_host_check")
    src = os.path.join(ROOT, "tests", "native", "jpeg_host_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", src, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "jpeg host checks ok" in res.stdout
