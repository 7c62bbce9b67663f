"""Compile and run tests/cpp/read_test.cc: RAMCloud::ReplayTable::multiRead
(include/ramcloud/Crc32CBatch.h) as a master answers a multi-read from the
table it recovers into: add per arriving batch after deviceReplayVerify, one
request answered after each add, with and without a limit."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_read_test(ramcrc, tmp_path):
    exe = tmp_path / "read_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "read_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_read_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::multiRead compiles into a host program (hipcc,
    for hipMalloc) against the C ABI."""
    assert _build_read_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_read_gpu(ramcrc, tmp_path):
    """Two batches through the C++ class: verify -> add -> multiRead per batch;
    reply, part offsets, results and summary equal the host form's byte for
    byte, and every part carries its key's value."""
    exe = _build_read_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
