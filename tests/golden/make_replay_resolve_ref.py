"""Generate tests/golden/replay_resolve_ref.json.

The object and tombstone cases of the reference's ObjectManagerTest.replaySegment
(src/ObjectManagerTest.cc:887-1191) as data, in our own words: per case the
records of one key in the order the test replays them -- what the test plants
in the hash table beforehand comes first, as the record that put it there --
and what its lookups find afterwards.  Five cases for objects (:915-1013) and
five for tombstones (:1030-1190); the tombstone case 1b replays two keys
(:1048-1067 at an equal version, :1069-1087 over an older object), so it is
two entries here.  Nothing is compiled or copied from the reference; the
survivors are the test's EXPECT lines, and the sequential replay of
tests/resolve_cases.py is asserted to agree before anything is written.

Usage:  python tests/golden/make_replay_resolve_ref.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import resolve_cases as rc  # noqa: E402

O, T = "OBJ", "OBJTOMB"

# (name, source lines, what it shows, [(type, key, version)], survivor (type, version, index))
CASES = [
    ("object 1a", "915-930", "a newer object is there: the older one is ignored",
     [(O, "key0", 1), (O, "key0", 0)], (O, 1, 0)),
    ("object 1b", "932-945", "an older object is there: it is replaced",
     [(O, "key1", 0), (O, "key1", 1)], (O, 1, 1)),
    ("object 2a", "947-973", "a tombstone of an equal or newer version is there: objects are ignored",
     [(T, "key2", 1), (O, "key2", 1), (O, "key2", 0)], (T, 1, 0)),
    ("object 2b", "975-1003", "a tombstone of a lesser version is there: the object replaces it",
     [(T, "key3", 10), (O, "key3", 11)], (O, 11, 1)),
    ("object 3", "1005-1013", "nothing is there: the object is added",
     [(O, "key4", 0)], (O, 0, 0)),
    ("tombstone 1a", "1030-1045", "a newer object is there: the tombstone is ignored",
     [(O, "key5", 1), (T, "key5", 0)], (O, 1, 0)),
    ("tombstone 1b (equal version)", "1047-1067", "an object of the same version is there: it goes",
     [(O, "key6", 0), (T, "key6", 0)], (T, 0, 1)),
    ("tombstone 1b (older object)", "1069-1087", "an older object is there: it goes",
     [(O, "key7", 0), (T, "key7", 1)], (T, 1, 1)),
    ("tombstone 2a", "1089-1124", "a newer tombstone is there: the older one is ignored",
     [(T, "key8", 1), (T, "key8", 0)], (T, 1, 0)),
    ("tombstone 2b", "1126-1163", "an older tombstone is there: it is replaced",
     [(T, "key9", 0), (T, "key9", 1)], (T, 1, 1)),
    ("tombstone 3", "1165-1190", "nothing is there: the tombstone is added",
     [(T, "key10", 0)], (T, 0, 0)),
]


def main():
    code = {O: rc.OBJ, T: rc.OBJTOMB}
    cases = []
    for name, lines, about, records, (st, sv, si) in CASES:
        parts = [("rec", code[t], (0, k.encode()), v) for t, k, v in records]
        (ver, etype, rec), = rc.replay(parts).values()
        assert (etype, ver, rec) == (code[st], sv, si), name
        cases.append({"name": name, "lines": lines, "about": about,
                      "records": [list(r) for r in records],
                      "survivor": {"type": st, "version": sv, "index": si}})
    ref = {"source": "src/ObjectManagerTest.cc:887-1191 (TEST_F(ObjectManagerTest, replaySegment))",
           "table_id": 0, "cases": cases}
    out = os.path.join(HERE, "replay_resolve_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(cases), "cases")


if __name__ == "__main__":
    main()
