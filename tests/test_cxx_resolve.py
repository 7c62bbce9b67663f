"""Compile and run tests/cpp/resolve_test.cc: Crc32CBatch::deviceReplayResolve
(include/ramcloud/Crc32CBatch.h) as a recovery master calls it after
deviceReplayVerify, before deviceRecoveryAppend with one partition."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_resolve_test(ramcrc, tmp_path):
    exe = tmp_path / "resolve_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "resolve_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_resolve_wrapper_builds(ramcrc, tmp_path):
    """Crc32CBatch::deviceReplayResolve compiles into a host program
    (hipcc, for hipMalloc) against the C ABI."""
    assert _build_resolve_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_resolve_wrapper_gpu(ramcrc, tmp_path):
    """verify -> partition (for its hashes) -> resolve -> append through the
    C++ wrappers: winners, live list and counters against the host form, with
    given and with computed hashes; the appended entry counts are the list's;
    a segment with a wrong certificate takes no part."""
    exe = _build_resolve_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
