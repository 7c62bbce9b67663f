"""Generate tests/golden/key_hash_ref.json (run in the build container only).

Key::getHash (src/Key.cc:140-151) as data: (table id, key hex, hash) cases
computed by the reference's own MurmurHash3.cc, compiled into a temporary
directory outside the tree (nothing compiled from the reference is kept, and
neither build(), the tests nor the bench call this script).  Before anything
is written, the three hashes the reference's tests hold as constants are
checked: Key(82, "hey-hey-hey", 12) = 0x889d47d556739eeb (src/KeyTest.cc:95-101)
and the hashes of (1, "1") and (1, "2") that
src/RecoverySegmentBuilderTest.cc:246-268 prints.

Cases, in this order: the three constants; every key length 0 .. 64, the table
ids 0, 1, 82, 2^32 + 1 and 2^64 - 1 in turn (the seed is the low 32 bits of the
table id); lengths 255, 256, 4,095 and 65,535; 200 random keys of up to 48
bytes under random table ids.

Usage:  python tests/golden/make_key_hash_ref.py [path to the reference's src]
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_IDS = [0, 1, 82, (1 << 32) + 1, (1 << 64) - 1]

SHIM = """
#include <stdint.h>
#include "MurmurHash3.h"
extern "C" uint64_t ref_key_hash(uint64_t table_id, const void* key, int len)
{
    uint64_t out[2];
    RAMCloud::MurmurHash3_x64_128(key, len, static_cast<uint32_t>(table_id), &out);
    return out[0];
}
"""


def load_reference(src):
    tmp = tempfile.mkdtemp(prefix="key_hash_ref_")
    shim = os.path.join(tmp, "shim.cc")
    with open(shim, "w") as f:
        f.write(SHIM)
    lib = os.path.join(tmp, "libkeyhash.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I" + src, shim,
                           os.path.join(src, "MurmurHash3.cc"), "-o", lib])
    L = ctypes.CDLL(lib)
    L.ref_key_hash.restype = ctypes.c_uint64
    L.ref_key_hash.argtypes = [ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int]
    return lambda table_id, key: int(L.ref_key_hash(table_id, bytes(key), len(key)))


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RAMCLOUD_SRC", "")
    if not os.path.exists(os.path.join(src, "MurmurHash3.cc")):
        sys.exit("give the reference's src directory (argument or RAMCLOUD_SRC)")
    h = load_reference(src)
    assert h(82, b"hey-hey-hey\0") == 0x889d47d556739eeb
    assert h(1, b"1") == 0xDD5D9F7F60D5B056
    assert h(1, b"2") == 0x3554F985FBED3C16
    rng = np.random.default_rng(20260)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    cases = [[82, b"hey-hey-hey\0"], [1, b"1"], [1, b"2"]]
    cases += [[TABLE_IDS[n % 5], rand(n)] for n in range(65)]
    cases += [[TABLE_IDS[(i + 3) % 5], rand(n)] for i, n in enumerate((255, 256, 4095, 65535))]
    for _ in range(200):
        t = int(rng.integers(0, 1 << 63)) if rng.random() < 0.5 else int(rng.integers(0, 1000))
        cases.append([t, rand(int(rng.integers(0, 49)))])
    out = {"_source": __doc__.strip().splitlines()[0],
           "cases": [[t, k.hex(), h(t, k)] for t, k in cases]}
    path = os.path.join(HERE, "key_hash_ref.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(f"wrote {len(cases)} cases to {path}")


if __name__ == "__main__":
    main()
