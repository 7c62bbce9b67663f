"""Compile and run tests/cpp/lookup_test.cc: RAMCloud::ReplayTable::lookup
(include/ramcloud/Crc32CBatch.h) as a master serves a multi-read from the table
it recovers into: add per arriving batch after deviceReplayVerify, a batch of
keys looked up after each add."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_lookup_test(ramcrc, tmp_path):
    exe = tmp_path / "lookup_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "lookup_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_lookup_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::lookup compiles into a host program (hipcc, for
    hipMalloc) against the C ABI."""
    assert _build_lookup_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_lookup_gpu(ramcrc, tmp_path):
    """Two batches through the C++ class: verify -> add -> lookup per batch;
    results and counts equal the host form's byte for byte, and every object's
    value lies where the answer says."""
    exe = _build_lookup_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
