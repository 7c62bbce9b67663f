"""Compile and run tests/cpp/append_test.cc: Crc32CBatch::deviceRecoveryAppend
(include/ramcloud/Crc32CBatch.h) as a backup calls it after deviceReplayVerify."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_append_test(ramcrc, tmp_path):
    exe = tmp_path / "append_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "append_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_append_wrapper_builds(ramcrc, tmp_path):
    """Crc32CBatch::deviceRecoveryAppend compiles into a host program (hipcc,
    for hipMalloc) against the C ABI."""
    assert _build_append_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_append_wrapper_gpu(ramcrc, tmp_path):
    """The C++ append wrapper on the device: bytes, certificates and counts of
    six recovery segments against Segment::append restated with the drop-in
    Crc32C; the outputs of a replica with a wrong certificate stay empty."""
    exe = _build_append_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
