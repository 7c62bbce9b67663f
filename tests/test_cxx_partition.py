"""Compile and run tests/cpp/partition_test.cc: Crc32CBatch::deviceRecoveryPartition
(include/ramcloud/Crc32CBatch.h) as a backup calls it between deviceReplayVerify
and deviceRecoveryAppend."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_partition_test(ramcrc, tmp_path):
    exe = tmp_path / "partition_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "partition_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_partition_wrapper_builds(ramcrc, tmp_path):
    """Crc32CBatch::deviceRecoveryPartition compiles into a host program
    (hipcc, for hipMalloc) against the C ABI."""
    assert _build_partition_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_partition_wrapper_gpu(ramcrc, tmp_path):
    """walk -> partition -> append through the C++ wrappers: the list, hashes
    and counters against the host form and the reference test's hashes; the
    appended entry counts are the list's; a replica with a wrong certificate
    places nothing."""
    exe = _build_partition_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
