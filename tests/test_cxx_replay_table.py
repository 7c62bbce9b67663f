"""Compile and run tests/cpp/replay_table_test.cc: RAMCloud::ReplayTable
(include/ramcloud/Crc32CBatch.h) as a recovery master drives it: add per
arriving batch after deviceReplayVerify, then live and deviceRecoveryAppend
with one partition per batch."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_replay_table_test(ramcrc, tmp_path):
    exe = tmp_path / "replay_table_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "replay_table_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_replay_table_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable compiles into a host program (hipcc, for
    hipMalloc) against the C ABI."""
    assert _build_replay_table_test(ramcrc, tmp_path).exists()


@pytest.mark.gpu
def test_cxx_replay_table_gpu(ramcrc, tmp_path):
    """Two batches through the C++ class: verify -> add per batch, the live
    query of every batch after each add against the host table, stats, then
    live -> append per batch; the appended entry counts are the lists'; reset
    empties the table."""
    exe = _build_replay_table_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
