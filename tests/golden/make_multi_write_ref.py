"""Generate tests/golden/multi_write_ref.json.

What the reference's own tests say about a write, as data in our own words.
Every step is one multi-write call; the table a step sees is what the earlier
steps' entries, walked and added, have made of it.

  - ObjectManagerTest.writeObject (src/ObjectManagerTest.cc:1620-1636): key "1"
    with value "value" in table 1.  A new object is 33 bytes at version 1; an
    overwrite is 33 bytes at version 2 plus a 33-byte tombstone of version 1,
    byteCount 99 over 3 records; a write over a tombstone succeeds.  The
    reference stores that tombstone into its hash table in place of the
    object; a replay table keeps the higher version, so ours carries version
    2, which beats the object of version 2.
  - MasterServiceTest.multiWrite_basics (src/MasterServiceTest.cc:1616-1640):
    after one write of key "1", a multi-write of "0" and "1" returns versions
    2 and 2: "0" takes the next allocated version, "1" its old version plus 1.
  - multiWrite_rejectRules (:1642-1651): doesntExist on an empty table gives
    STATUS_OBJECT_DOESNT_EXIST (3) with VERSION_NONEXISTENT (0).
  - write_basics (:3902-3941): versions 1, 2, 3 of one key.
  - write_safeVersionNumberUpdate (:3943-3986): versions 1, 2, 29, 3 with the
    safe version 2, 2, 30, 30 after each write (the test sets it to 29 before
    the third).

Nothing is compiled or copied from the reference; the plain-Python expectation
of tests/write_cases.py is asserted to agree before anything is written.

Usage:  python tests/golden/make_multi_write_ref.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

OK, DOESNT_EXIST = 0, 3


def step(objects, next_version, status, version, **kw):
    return dict(objects=objects, next_version=next_version, status=status, version=version, **kw)


SCENARIOS = [
    dict(name="writeObject", lines="src/ObjectManagerTest.cc:1620-1636", steps=[
        step([[1, "1", "value"]], 1, [OK], [1], entry_bytes=[33],
             summary=dict(ok=1, tombstones=0, object_bytes=33, tombstone_bytes=0, next_version=2)),
        step([[1, "1", "value"]], 2, [OK], [2], entry_bytes=[33, 33],
             summary=dict(ok=1, tombstones=1, object_bytes=33, tombstone_bytes=33, next_version=2)),
        dict(tombstone=[1, "1", 2]),
        step([[1, "1", "value"]], 2, [OK], [3], entry_bytes=[33],
             summary=dict(ok=1, tombstones=0, allocated=1, next_version=4)),
    ]),
    dict(name="multiWrite_basics", lines="src/MasterServiceTest.cc:1616-1640", steps=[
        step([[1, "1", "originalVal\0"]], 1, [OK], [1]),
        step([[1, "0", "firstVal"], [1, "1", "secondVal"]], 2, [OK, OK], [2, 2],
             summary=dict(ok=2, tombstones=1, allocated=1, next_version=3)),
    ]),
    dict(name="multiWrite_rejectRules", lines="src/MasterServiceTest.cc:1642-1651", steps=[
        step([[1, "key0", "item0"]], 1, [DOESNT_EXIST], [0], rules=[dict(doesnt_exist=1)],
             summary=dict(ok=0, doesnt_exist=1, out_bytes=0, allocated=0, next_version=1)),
    ]),
    dict(name="write_basics", lines="src/MasterServiceTest.cc:3902-3941", steps=[
        step([[1, "key0", "item0"]], 1, [OK], [1], entry_bytes=[36]),
        step([[1, "key0", "item0-v2"]], 2, [OK], [2]),
        step([[1, "key0", "item0-v3"]], 2, [OK], [3]),
    ]),
    dict(name="write_safeVersionNumberUpdate", lines="src/MasterServiceTest.cc:3943-3986", steps=[
        step([[1, "k0", "value0"]], 1, [OK], [1], summary=dict(next_version=2)),
        step([[1, "k0", "value1"]], 2, [OK], [2], summary=dict(next_version=2)),
        step([[1, "k1", "value3"]], 29, [OK], [29], summary=dict(next_version=30)),
        step([[1, "k0", "value4"]], 30, [OK], [3], summary=dict(next_version=30)),
    ]),
]


def main():
    ref = {"source": "src/ObjectManagerTest.cc:1620-1636 (writeObject), src/MasterServiceTest.cc:1616-1651 "
                     "(multiWrite_*), :3902-3986 (write_*)",
           "scenarios": SCENARIOS,
           "steps": sum(1 for sc in SCENARIOS for st in sc["steps"] if "objects" in st)}
    from oracle import oracle
    oracle.lib()
    import write_cases as wc
    assert wc.check_expectation_against_golden(oracle, ref) == ref["steps"]
    out = os.path.join(HERE, "multi_write_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(SCENARIOS), "scenarios,", ref["steps"], "steps")


if __name__ == "__main__":
    main()
