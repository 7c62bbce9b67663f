"""Compile and run tests/cpp/remove_test.cc: RAMCloud::ReplayTable::multiRemove
(include/ramcloud/Crc32CBatch.h) as a master serves a multi-remove from the
table it recovered into: remove, walk the output with its certificate, add it,
and read every key with multiRead."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_remove_test(ramcrc, tmp_path):
    exe = tmp_path / "remove_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "remove_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_remove_builds_and_validates_arguments(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::multiRemove compiles into a host program (hipcc,
    for hipMalloc) against the C ABI; without a GPU the program checks what
    both forms refuse and the host form against an empty table."""
    exe = _build_remove_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe), "--cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout


@pytest.mark.gpu
def test_cxx_remove_gpu(ramcrc, tmp_path):
    """One batch through the C++ class, then multiRemove -> verify -> add ->
    multiRead: every output equals the host form's byte for byte, the output
    passes the walk and the checksum pass, and no removed key reads back."""
    exe = _build_remove_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
