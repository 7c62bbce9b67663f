"""Compile and run tests/cpp/clean_test.cc: RAMCloud::ReplayTable::clean and
cleanSize (include/ramcloud/Crc32CBatch.h) as a master's cleaner uses them:
size the survivor, clean a batch out of the table, hand its arrays back, and
read every key."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_clean_test(ramcrc, tmp_path):
    exe = tmp_path / "clean_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "clean_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def test_cxx_clean_builds_and_runs_the_host_form(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::clean compiles into a host program (hipcc, for
    hipMalloc) against the C ABI; without a GPU the program checks what both
    forms refuse and the host form: the summary, the retired batch, and every
    key's answer before and after with the victim's arrays overwritten."""
    exe = _build_clean_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe), "--cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout


@pytest.mark.gpu
def test_cxx_clean_gpu(ramcrc, tmp_path):
    """Two batches through the C++ class, then cleanSize -> clean: every output
    equals the host form's byte for byte, deviceReplayVerify over the survivor
    writes the call's status and record table, and with the victim's arrays
    overwritten a multiRead of every key returns the host form's reply."""
    exe = _build_clean_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
