"""Compile and run tests/cpp/write_test.cc: RAMCloud::ReplayTable::multiWrite
(include/ramcloud/Crc32CBatch.h) as a master serves a multi-write from the
table it recovered into: write, walk the output with its certificate, add it,
and read every key back with multiRead."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_write_test(ramcrc, tmp_path):
    exe = tmp_path / "write_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "write_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_write_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::multiWrite compiles into a host program (hipcc,
    for hipMalloc) against the C ABI."""
    assert _build_write_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_write_gpu(ramcrc, tmp_path):
    """One batch through the C++ class, then multiWrite -> verify -> add ->
    multiRead: every output equals the host form's byte for byte, the output
    passes the walk and the checksum pass, and every written key reads back."""
    exe = _build_write_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
