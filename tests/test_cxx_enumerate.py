"""Compile and run tests/cpp/enumerate_test.cc: RAMCloud::ReplayTable::enumerate
(include/ramcloud/Crc32CBatch.h) as a master answers ENUMERATE from the table it
recovers into: add per arriving batch after deviceReplayVerify, the table
enumerated from cursor (0, 0) to its end after each add.  And
tests/cpp/enumerate_host_test.cc: the host form driven by a stand-alone
host-only program, run plain and as a sanitizer build of ramcrc_host.cc."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_enumerate_test(ramcrc, tmp_path):
    exe = tmp_path / "enumerate_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "enumerate_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def _host_program(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror",
        "-Wno-unused-function"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ramcloud_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "enumerate_host_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "csrc", "ramcrc_host.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
    return out


def test_cxx_enumerate_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::enumerate compiles into a host program (hipcc,
    for hipMalloc) against the C ABI."""
    assert _build_enumerate_test(ramcrc, tmp_path).exists()


def test_cxx_enumerate_host_program(tmp_path):
    """The host form alone, compiled from ramcrc_host.cc without the library or
    a GPU: buckets of 1, 2, 3 and 40 keys in one and three adds, the cut at
    every entry's start and end, the cursor walk, stale frames."""
    _host_program(tmp_path, "enumerate_host_test", [])


def test_cxx_enumerate_host_program_sanitized(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined, on
    the CPU: its payloads, frames and summaries lie in exactly sized blocks at
    odd addresses, so a byte past an end or a misaligned typed access of the
    host form ends the run."""
    out = _host_program(tmp_path, "enumerate_host_test_san",
                        ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


@pytest.mark.gpu
def test_cxx_enumerate_gpu(ramcrc, tmp_path):
    """Two batches through the C++ class: verify -> add -> enumerate per batch;
    payload and summary of every call equal the host form's byte for byte, and
    every entry carries its key's value."""
    exe = _build_enumerate_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
