"""Memory safety of the field lists behind the optional stages of the C ABI (csrc/io_fields.hpp: the carve and copy helpers
every stage's layout and copy-back go through): tests/native/io_fields_check.cpp is built as a stand-alone program with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own.  Nothing loaded into python runs under a
sanitizer."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_field_lists_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "io_fields_check")
    src = os.path.join(ROOT, "tests", "native", "io_fields_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", src, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "io field checks ok" in res.stdout
