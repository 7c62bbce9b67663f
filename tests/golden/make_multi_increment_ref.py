"""Generate tests/golden/multi_increment_ref.json.

What the reference's own tests say about an increment, as data in our own
words.  A step stores objects (each [table id, key, the value's bytes in hex,
version]) as a batch of its own, or increments keys in one multi-increment call
(args: [add_int64, add_double] per key); the table a step sees is what the
earlier steps' entries, walked and added, have made of it.  A value is an
integer, {"double": x}, or null where the reference's test does not look.

  - MasterServiceTest.increment_basic (src/MasterServiceTest.cc:675-701): key0
    holds the int64 1 at version 1; incremented by 2 it is 3 at version 2, and a
    read returns those 8 bytes.  key1 holds the double 1.0 at version 2;
    incremented by 2.0 it is 3.0 at version 3.
  - increment_create (:731-751): on an empty table, key0 + 1 creates 1 at
    version 1; key1 + 1.0 creates 1.0 at version 2; key2 + 0 creates 0 at
    version 3 (a zero increment still writes); key2 + 0.0 is 0.0 at version 4.
  - increment_rejectRules (:753-776): doesntExist on the absent key0 gives
    STATUS_OBJECT_DOESNT_EXIST (3); exists on the written key1 gives
    STATUS_OBJECT_EXISTS (4); key2, written at version 2 and incremented to
    version 3, against versionNeGiven with given version 2 gives
    STATUS_WRONG_VERSION (5).
  - increment_invalidObject (:815-826): a 4-byte int32 and a 4-byte float give
    STATUS_INVALID_OBJECT (22) for the integer and the double increment.
  - multiIncrement_basics (:1364-1377): one call, key "0" + 1 and key "1" +
    1.0 on an empty table: both OK, 1 and 1.0, the versions add up to 3.
  - multiIncrement_rejectRules (:1379-1388): doesntExist on an empty table
    gives STATUS_OBJECT_DOESNT_EXIST with VERSION_NONEXISTENT (0).

Ours, not the reference's: the version of a rejected part (the object's) and
the third field of a part that is not OK (the bits of add_double).

Nothing is compiled or copied from the reference; the plain-Python expectation
of tests/increment_cases.py is asserted to agree before anything is written.

Usage:  python tests/golden/make_multi_increment_ref.py
"""
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

OK, DOESNT_EXIST, EXISTS, WRONG_VERSION, INVALID_OBJECT = 0, 3, 4, 5, 22


def int64(x):
    return struct.pack("<q", x).hex()


def double(x):
    return struct.pack("<d", x).hex()


def inc(keys, args, next_version, status, version, **kw):
    return dict(keys=keys, args=args, next_version=next_version, status=status, version=version, **kw)


NOTHING = dict(ok=0, out_bytes=0, tombstones=0, allocated=0)

SCENARIOS = [
    dict(name="increment_basic", lines="src/MasterServiceTest.cc:675-701", steps=[
        dict(objects=[[1, "key0", int64(1), 1]]),
        inc([[1, "key0"]], [[2, 0.0]], 2, [OK], [2], value=[3],
            summary=dict(ok=1, created=0, tombstones=1, allocated=0, next_version=2)),
        dict(objects=[[1, "key1", double(1.0), 2]]),
        inc([[1, "key1"]], [[0, 2.0]], 3, [OK], [3], value=[{"double": 3.0}],
            summary=dict(ok=1, tombstones=1, next_version=3)),
    ]),
    dict(name="increment_create", lines="src/MasterServiceTest.cc:731-751", steps=[
        inc([[1, "key0"]], [[1, 0.0]], 1, [OK], [1], value=[1],
            summary=dict(ok=1, created=1, tombstones=0, allocated=1, next_version=2)),
        inc([[1, "key1"]], [[0, 1.0]], 2, [OK], [2], value=[{"double": 1.0}], summary=dict(created=1, next_version=3)),
        inc([[1, "key2"]], [[0, 0.0]], 3, [OK], [3], value=[0],
            summary=dict(ok=1, created=1, out_bytes=41, next_version=4)),
        inc([[1, "key2"]], [[0, 0.0]], 4, [OK], [4], value=[{"double": 0.0}],
            summary=dict(ok=1, created=0, tombstones=1, next_version=4)),
    ]),
    dict(name="increment_rejectRules", lines="src/MasterServiceTest.cc:753-776", steps=[
        inc([[1, "key0"]], [[1, 0.0]], 1, [DOESNT_EXIST], [0], rules=[dict(doesnt_exist=1)], value=[0],
            summary=dict(NOTHING, doesnt_exist=1, next_version=1)),
        dict(objects=[[1, "key1", int64(0), 1]]),
        inc([[1, "key1"]], [[1, 0.0]], 2, [EXISTS], [1], rules=[dict(exists=1)],
            summary=dict(NOTHING, object_exists=1, next_version=2)),
        dict(objects=[[1, "key2", int64(0), 2]]),
        inc([[1, "key2"]], [[1, 0.0]], 3, [OK], [3], value=[1]),
        inc([[1, "key2"]], [[1, 0.0]], 3, [WRONG_VERSION], [3], rules=[dict(version_ne_given=1, given_version=2)],
            summary=dict(NOTHING, wrong_version=1, next_version=3)),
    ]),
    dict(name="increment_invalidObject", lines="src/MasterServiceTest.cc:815-826", steps=[
        dict(objects=[[1, "key0", "00000000", 1]]),
        inc([[1, "key0"]], [[1, 0.0]], 2, [INVALID_OBJECT], [1], summary=dict(NOTHING, invalid_object=1)),
        dict(objects=[[1, "key1", struct.pack("<f", 0.0).hex(), 2]]),
        inc([[1, "key1"]], [[0, 1.0]], 3, [INVALID_OBJECT], [2], value=[{"double": 1.0}],
            summary=dict(NOTHING, invalid_object=1, next_version=3)),
    ]),
    dict(name="multiIncrement_basics", lines="src/MasterServiceTest.cc:1364-1377", steps=[
        inc([[1, "0"], [1, "1"]], [[1, 0.0], [0, 1.0]], 1, [OK, OK], [1, 2], value=[1, {"double": 1.0}],
            summary=dict(ok=2, created=2, allocated=2, next_version=3, value_bytes=16, key_bytes=8)),
    ]),
    dict(name="multiIncrement_rejectRules", lines="src/MasterServiceTest.cc:1379-1388", steps=[
        inc([[1, "key0"]], [[1, 0.0]], 1, [DOESNT_EXIST], [0], rules=[dict(doesnt_exist=1)],
            summary=dict(NOTHING, doesnt_exist=1, next_version=1)),
    ]),
]


def main():
    ref = {"source": "src/MasterServiceTest.cc:675-701, :731-776, :815-826 (increment_*), :1364-1388 "
                     "(multiIncrement_*)",
           "scenarios": SCENARIOS,
           "steps": sum(1 for sc in SCENARIOS for st in sc["steps"] if "keys" in st)}
    from oracle import oracle
    oracle.lib()
    import increment_cases as ic
    assert ic.check_expectation_against_golden(oracle, ref) == ref["steps"]
    out = os.path.join(HERE, "multi_increment_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(SCENARIOS), "scenarios,", ref["steps"], "steps")


if __name__ == "__main__":
    main()
