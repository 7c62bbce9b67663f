"""Compile and run tests/cpp/index_test.cc: RAMCloud::ReplayTable::buildIndex
and lookupIndexKeys (include/ramcloud/Crc32CBatch.h) as a master serves an
indexed read from the table it recovers into: add per arriving batch after
deviceReplayVerify, then build, lookup and readHashes on one stream.  And
tests/cpp/index_host_test.cc: the host forms driven by a stand-alone host-only
program, run plain and as a sanitizer build of ramcrc_host.cc."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_index_test(ramcrc, tmp_path):
    exe = tmp_path / "index_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "index_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def _host_program(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror",
        "-Wno-unused-function"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ramcloud_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "index_host_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "csrc", "ramcrc_host.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
    return out


def test_cxx_index_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::buildIndex and lookupIndexKeys compile into a
    host program (hipcc, for hipMalloc) against the C ABI."""
    assert _build_index_test(ramcrc, tmp_path).exists()


def test_cxx_index_host_program(tmp_path):
    """The host forms alone, compiled from ramcrc_host.cc without the library
    or a GPU: two batches with overwrites and removes, three index ids, the
    sizing call and both capacities one short, every point query, ranges with
    max_hashes and first_allowed_hash, the output cut at many capacities, a
    bad query."""
    _host_program(tmp_path, "index_host_test", [])


def test_cxx_index_host_program_sanitized(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined, on
    the CPU: its arrays lie in exactly sized blocks at odd addresses, so a byte
    past an end or a misaligned typed access of the host forms ends the run."""
    out = _host_program(tmp_path, "index_host_test_san",
                        ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


@pytest.mark.gpu
def test_cxx_index_gpu(ramcrc, tmp_path):
    """Two batches through the C++ class: verify -> add -> buildIndex ->
    lookupIndexKeys -> readHashes per batch; entries, hashes, results and
    summaries equal the host forms', and every object read back carries a
    second key inside the asked range."""
    exe = _build_index_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
