"""Compile and run tests/cpp/read_hashes_test.cc: RAMCloud::ReplayTable::readHashes
(include/ramcloud/Crc32CBatch.h) as a master answers READ_HASHES from the table
it recovers into: add per arriving batch after deviceReplayVerify, one indexed
read answered after each add, with and without a limit.  And
tests/cpp/read_hashes_host_test.cc: the host form driven by a stand-alone
host-only program, the one a sanitizer build of ramcrc_host.cc runs."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_read_hashes_test(ramcrc, tmp_path):
    exe = tmp_path / "read_hashes_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "read_hashes_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_read_hashes_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::readHashes compiles into a host program (hipcc,
    for hipMalloc) against the C ABI."""
    assert _build_read_hashes_test(ramcrc, tmp_path).exists()


def test_cxx_read_hashes_host_program(tmp_path):
    """The host form alone, compiled from ramcrc_host.cc without the library or
    a GPU: fan-out of 1, 2, 3 and 40 keys under one caller hash in one and
    three adds, and the cut at every hash's start and end."""
    exe = tmp_path / "read_hashes_host_test"
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror",
        "-Wno-unused-function",
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ramcloud_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "read_hashes_host_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "csrc", "ramcrc_host.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout


@pytest.mark.gpu
def test_cxx_read_hashes_gpu(ramcrc, tmp_path):
    """Two batches through the C++ class: verify -> add -> readHashes per batch;
    reply, parts and summary equal the host form's byte for byte, and every
    object part carries its key's value."""
    exe = _build_read_hashes_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
