"""Compile and run tests/cpp/sidelog_test.cc: Crc32CBatch::deviceReplaySideLog
(include/ramcloud/Crc32CBatch.h) as a recovery master calls it after
deviceReplayVerify."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_sidelog_test(ramcrc, tmp_path):
    exe = tmp_path / "sidelog_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "sidelog_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_sidelog_wrapper_builds(ramcrc, tmp_path):
    """Crc32CBatch::deviceReplaySideLog compiles into a host program (hipcc,
    for hipMalloc) against the C ABI."""
    assert _build_sidelog_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_sidelog_wrapper_gpu(ramcrc, tmp_path):
    """The C++ side-log wrapper on the device over one mixed case: bytes,
    certificates, references and counts of two side-log segments against
    Segment::append restated with the drop-in Crc32C, every tombstone
    rewritten; the second segment fills up."""
    exe = _build_sidelog_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
