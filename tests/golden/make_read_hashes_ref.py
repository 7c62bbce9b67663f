"""Generate tests/golden/read_hashes_ref.json.

What the reference's own tests say about an indexed read (READ_HASHES), as
data in our own words:

  - ObjectManagerTest.readHashes (src/ObjectManagerTest.cc:497-566): two
    two-key objects in table 0, the primary-key hashes of both asked with
    maxLength 1000; it expects 2 hashes, 2 objects, and per object the layout
    version (8 bytes), length (4 bytes), keys and value, whose value reads
    "obj0value" and "obj1value";
  - MasterServiceTest.readHashes (src/MasterServiceTest.cc:1852-1896): one
    two-key object in table 1, asked by the constant the test itself states,
    Key::getHash(1, "obj0key0", 8) = 4921604586378860710; it expects 1 hash, 1
    object, version 1 (a table's first write) and the value "obj0value";
  - RamCloudTest.readHashes (src/RamCloudTest.cc:775-845): three two-key
    objects, their three primary-key hashes in order; it expects 3 objects
    with the values "valueA", "valueB", "valueC" in that order.  (The test's
    table id comes from createTable; 1 stands for it here.)

A version the reference's test does not look at is the one its writes give (a
table's writes get 1, 2, 3) and is marked "checked": false.  The length of a
part is that of the keys and value: key count, one cumulative length per key,
the keys, the value.  Nothing is compiled or copied from the reference; the
project's plain-Python Key::getHash (tests/partition_cases.py) is asserted to
give the stated constant before anything is written.

Usage:  python tests/golden/make_read_hashes_ref.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import partition_cases as pc  # noqa: E402

# keys and value of an object: key count, cumulative lengths, the keys, the value
kv = lambda keys, value: 1 + 2 * len(keys) + sum(len(k) for k in keys) + len(value)


def obj(keys, value, version, checked):
    return dict(keys=keys, value=value, version=version, version_checked=checked, length=kv(keys, value))


SCENARIOS = [
    dict(name="ObjectManagerTest.readHashes", lines="src/ObjectManagerTest.cc:497-566", table_id=0,
         objects=[obj(["obj0key0", "obj0key1"], "obj0value", 1, False),
                  obj(["obj1key0", "obj1key1"], "obj1value", 2, False)],
         ask=["obj0key0", "obj1key0"], max_length=1000, hashes=2, objects_returned=2, order=[0, 1]),
    dict(name="MasterServiceTest.readHashes", lines="src/MasterServiceTest.cc:1852-1896", table_id=1,
         objects=[obj(["obj0key0", "obj0key1"], "obj0value", 1, True)],
         ask=["obj0key0"], ask_hashes=[4921604586378860710], max_length=None, hashes=1,
         objects_returned=1, order=[0]),
    dict(name="RamCloudTest.readHashes", lines="src/RamCloudTest.cc:775-845", table_id=1,
         objects=[obj(["keyA0", "keyA1"], "valueA", 1, False), obj(["keyB0", "keyB1"], "valueB", 2, False),
                  obj(["keyC0", "keyC1"], "valueC", 3, False)],
         ask=["keyA0", "keyB0", "keyC0"], max_length=None, hashes=3, objects_returned=3, order=[0, 1, 2]),
]

CONSTANTS = [dict(table_id=1, key="obj0key0", hash=4921604586378860710)]


def main():
    for c in CONSTANTS:
        assert pc.key_hash(c["table_id"], c["key"].encode()) == c["hash"], c
    assert kv(["obj0key0", "obj0key1"], "obj0value") == 1 + 4 + 16 + 9
    ref = {"source": "src/ObjectManagerTest.cc:497-566, src/MasterServiceTest.cc:1852-1896, "
                     "src/RamCloudTest.cc:775-845 (readHashes)",
           "part_header": {"version_bytes": 8, "length_bytes": 4},
           "key_hash_constants": CONSTANTS, "scenarios": SCENARIOS}
    out = os.path.join(HERE, "read_hashes_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(SCENARIOS), "scenarios")


if __name__ == "__main__":
    main()
