"""Compile and run tests/cpp/increment_test.cc:
RAMCloud::ReplayTable::multiIncrement (include/ramcloud/Crc32CBatch.h) as a
master serves a multi-increment from the table it recovered into: increment,
walk the output with its certificate, add it, and read every key with
multiRead."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_increment_test(ramcrc, tmp_path):
    exe = tmp_path / "increment_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "increment_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_increment_goldens_and_closed_loop_on_the_host(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::multiIncrement compiles into a host program
    (hipcc, for hipMalloc) against the C ABI; without a GPU the program takes
    the host form through what the reference's tests assert and through
    increment, walk, add, read, increment again, and checks what both forms
    refuse."""
    exe = _build_increment_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe), "--cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "goldens 0, closed loop 0; 0 mismatches" in out.stdout


@pytest.mark.gpu
def test_cxx_increment_gpu(ramcrc, tmp_path):
    """One batch through the C++ class, then multiIncrement -> verify -> add ->
    multiRead: every output equals the host form's byte for byte, the output
    passes the walk and the checksum pass, and every incremented key reads back
    its new 8 bytes."""
    exe = _build_increment_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
