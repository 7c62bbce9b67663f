"""Compile and run tests/cpp/migrate_test.cc: RAMCloud::ReplayTable::
migrateTablet (include/ramcloud/Crc32CBatch.h) as a master migrates a tablet
out of the table it serves from: add per arriving batch after
deviceReplayVerify, then the migration in one call and chained by the cursor,
and the receiving side's verify and add.  And tests/cpp/migrate_host_test.cc:
the host form driven by a stand-alone host-only program with its own
bookkeeping, run plain and as a sanitizer build of ramcrc_host.cc."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build_migrate_test(ramcrc, tmp_path):
    exe = tmp_path / "migrate_test"
    libdir = os.path.dirname(ramcrc.lib_path())
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-Werror",
        "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-I" + os.path.join(ROOT, "include", "ramcloud"),
        "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "migrate_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "dropin", "Crc32C.cc"),
        "-L" + libdir, "-lramcrc", "-Wl,-rpath," + libdir, "-o", str(exe)])
    return exe


def _host_program(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call([
        "/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror",
        "-Wno-unused-function"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ramcloud_amd", "csrc"),
        os.path.join(ROOT, "tests", "cpp", "migrate_host_test.cc"),
        os.path.join(ROOT, "ramcloud_amd", "csrc", "ramcrc_host.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
    return out


def test_cxx_migrate_builds(ramcrc, tmp_path):
    """RAMCloud::ReplayTable::migrateTablet compiles into a host program
    (hipcc, for hipMalloc) against the C ABI."""
    assert _build_migrate_test(ramcrc, tmp_path).exists()


def test_cxx_migrate_host_program(tmp_path):
    """The host form alone, compiled from ramcrc_host.cc without the library or
    a GPU: three batches with overwrites, a winning and a stale tombstone and
    an RPCRESULT record; both modes, six output capacities at every
    max_segments, hash ranges at their edges, every start cursor, d_sent at
    every length, the EINVAL list."""
    _host_program(tmp_path, "migrate_host_test", [])


def test_cxx_migrate_host_program_sanitized(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined, on
    the CPU: its outputs lie in exactly sized blocks at odd addresses, so a
    byte past an end or a misaligned typed access of the host form ends the
    run."""
    out = _host_program(tmp_path, "migrate_host_test_san",
                        ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


@pytest.mark.gpu
def test_cxx_migrate_gpu(ramcrc, tmp_path):
    """Three batches through the C++ class: verify -> add -> migrateTablet per
    arriving batch, in one call and chained, in both modes; every output equals
    the host form's, and the receiving table holds one key per sent record."""
    exe = _build_migrate_test(ramcrc, tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
