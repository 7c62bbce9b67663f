"""Generate tests/golden/multi_remove_ref.json.

What the reference's own tests say about a remove, as data in our own words.
A step stores objects (each [table id, key, value, version]) or a tombstone
([table id, key, version]) as a batch of its own, removes keys in one
multi-remove call, or reads a key; the table a step sees is what the earlier
steps' entries, walked and added, have made of it.

  - ObjectManagerTest.removeObject (src/ObjectManagerTest.cc:623-693): key "1"
    with value "hi" at version 93 in table 1, a 30-byte object.  Removing the
    absent key "2" is OK and writes nothing; with a tombstone stored for "2",
    removing it is OK and writes nothing; `exists` gives STATUS_OBJECT_EXISTS
    (4); the remove of "1" is OK with version 93 and a 33-byte tombstone
    (byteCount 63 -> 96), the safe version is 94 afterwards and a read answers
    STATUS_OBJECT_DOESNT_EXIST (3).  The tablet and lock cases before them are
    the caller's, answered before the call.
  - removeObject_returnRemovedObj (:695-722): key "a", the same object; the
    removed object is handed back (ours: the lookup's answer says where it
    lies), version 93, safe version 94, a read answers 3.
  - MasterServiceTest.multiRemove_basics (src/MasterServiceTest.cc:1519-1540):
    keys "0" and "1" written at versions 1 and 2; a multi-remove of both is OK
    with versions 1 and 2, a second one OK with version 0 twice.
  - multiRemove_rejectRules (:1542-1551): doesntExist on an empty table gives
    STATUS_OBJECT_DOESNT_EXIST with VERSION_NONEXISTENT (0).
  - remove_rejectRules (:2154-2165): versionNeGiven with given version 2
    against version 1 gives STATUS_WRONG_VERSION (5) with version 1.
  - remove_objectAlreadyDeletedRejectRules (:2221-2229): doesntExist against a
    key that is not there: status 3, version 0.
  - remove_objectAlreadyDeleted (:2231-2240): removing a key that never was is
    OK with version 0; so is the second remove of a key.

Nothing is compiled or copied from the reference; the plain-Python expectation
of tests/remove_cases.py is asserted to agree before anything is written.

Usage:  python tests/golden/make_multi_remove_ref.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

OK, DOESNT_EXIST, EXISTS, WRONG_VERSION = 0, 3, 4, 5
OBJECT, TOMBSTONE, ABSENT = 1, 2, 0


def remove(keys, next_version, status, version, **kw):
    return dict(keys=keys, next_version=next_version, status=status, version=version, **kw)


NOTHING = dict(removed=0, out_bytes=0, tombstone_bytes=0)

SCENARIOS = [
    dict(name="removeObject", lines="src/ObjectManagerTest.cc:623-693", steps=[
        dict(objects=[[1, "1", "hi", 93]], object_bytes=[30]),
        remove([[1, "2"]], 1, [OK], [0], old_kind=[ABSENT], summary=dict(NOTHING, ok_absent=1, next_version=1)),
        dict(tombstone=[1, "2", 4]),
        remove([[1, "2"]], 1, [OK], [0], old_kind=[TOMBSTONE], summary=dict(NOTHING, ok_absent=1, next_version=1)),
        remove([[1, "1"]], 1, [EXISTS], [93], rules=[dict(exists=1)],
               summary=dict(NOTHING, object_exists=1, next_version=1)),
        remove([[1, "1"]], 1, [OK], [93], entry_bytes=[33],
               summary=dict(removed=1, tombstone_bytes=33, out_bytes=35, next_version=94)),
        dict(read=[1, "1"], status=DOESNT_EXIST),
    ]),
    dict(name="removeObject_returnRemovedObj", lines="src/ObjectManagerTest.cc:695-722", steps=[
        dict(objects=[[1, "a", "hi", 93]], object_bytes=[30]),
        remove([[1, "a"]], 1, [OK], [93], entry_bytes=[33], old_kind=[OBJECT],
               summary=dict(removed=1, tombstone_bytes=33, next_version=94)),
        dict(read=[1, "a"], status=DOESNT_EXIST),
    ]),
    dict(name="multiRemove_basics", lines="src/MasterServiceTest.cc:1519-1540", steps=[
        dict(objects=[[1, "0", "firstVal", 1], [1, "1", "secondVal", 2]]),
        remove([[1, "0"], [1, "1"]], 3, [OK, OK], [1, 2], summary=dict(removed=2, next_version=3)),
        remove([[1, "0"], [1, "1"]], 3, [OK, OK], [0, 0], summary=dict(NOTHING, ok_absent=2, next_version=3)),
    ]),
    dict(name="multiRemove_rejectRules", lines="src/MasterServiceTest.cc:1542-1551", steps=[
        remove([[1, "key0"]], 1, [DOESNT_EXIST], [0], rules=[dict(doesnt_exist=1)],
               summary=dict(NOTHING, doesnt_exist=1, next_version=1)),
    ]),
    dict(name="remove_rejectRules", lines="src/MasterServiceTest.cc:2154-2165", steps=[
        dict(objects=[[1, "key0", "item0", 1]]),
        remove([[1, "key0"]], 2, [WRONG_VERSION], [1], rules=[dict(version_ne_given=1, given_version=2)],
               summary=dict(NOTHING, wrong_version=1, next_version=2)),
        dict(read=[1, "key0"], status=OK),
    ]),
    dict(name="remove_objectAlreadyDeletedRejectRules", lines="src/MasterServiceTest.cc:2221-2229", steps=[
        remove([[1, "key0"]], 1, [DOESNT_EXIST], [0], rules=[dict(doesnt_exist=1)],
               summary=dict(NOTHING, doesnt_exist=1)),
    ]),
    dict(name="remove_objectAlreadyDeleted", lines="src/MasterServiceTest.cc:2231-2240", steps=[
        remove([[1, "key1"]], 1, [OK], [0], summary=dict(NOTHING, ok_absent=1)),
        dict(objects=[[1, "key0", "item0", 1]]),
        remove([[1, "key0"]], 2, [OK], [1], entry_bytes=[36], summary=dict(removed=1, next_version=2)),
        remove([[1, "key0"]], 2, [OK], [0], summary=dict(NOTHING, ok_absent=1, next_version=2)),
    ]),
]


def main():
    ref = {"source": "src/ObjectManagerTest.cc:623-722 (removeObject*), src/MasterServiceTest.cc:1519-1551 "
                     "(multiRemove_*), :2154-2165 and :2221-2240 (remove_*)",
           "scenarios": SCENARIOS,
           "steps": sum(1 for sc in SCENARIOS for st in sc["steps"] if "keys" in st)}
    from oracle import oracle
    oracle.lib()
    import remove_cases as rm
    assert rm.check_expectation_against_golden(oracle, ref) == ref["steps"]
    out = os.path.join(HERE, "multi_remove_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(SCENARIOS), "scenarios,", ref["steps"], "steps")


if __name__ == "__main__":
    main()
