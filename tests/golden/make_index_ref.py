"""Generate tests/golden/index_ref.json.

What the reference's own tests say about an indexlet's range lookup
(LOOKUP_INDEX_KEYS) and about the order of secondary keys, as data in our own
words:

  - IndexletManagerTest.lookupIndexKeys_keyNotFound, _single, _multiple,
    _duplicate, _firstAllowedKeyHash and _largerThanMax
    (src/IndexletManagerTest.cc:661-867): the {key, pKHash} entries each test
    has inserted when it asks, its queries {first key, firstAllowedKeyHash,
    last key, maxNumHashes}, and what it expects: the hashes in order,
    nextKeyLength, the next key and nextKeyHash where it looks at them (null
    where it does not).  A test that inserts between its queries is one
    scenario per set of entries;
  - IndexKeyTest.keyCompare (src/IndexKeyTest.cc:29-41): its ten pairs with
    the sign it expects.  The last three involve an empty key and show that
    the reference's comparator is no order there: "" is below "abc", "abc" is
    below "", and "" is below "".

Nothing is compiled or copied from the reference.

Usage:  python tests/golden/make_index_ref.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

AIR, EARTH, FIRE = dict(key="air", hash=5678), dict(key="earth", hash=9876), dict(key="fire", hash=5432)
q = lambda first, last, hashes, fah=0, mx=100, **kw: dict(
    first=first, last=last, first_allowed_hash=fah, max_hashes=mx, hashes=hashes,
    next_key_length=kw.get("next_key_length"), next_key=kw.get("next_key"), next_key_hash=kw.get("next_key_hash"))

SCENARIOS = [
    dict(name="lookupIndexKeys_keyNotFound/empty", lines="src/IndexletManagerTest.cc:661-669", entries=[],
         queries=[q("air", "air", [])]),
    dict(name="lookupIndexKeys_keyNotFound/other", lines="src/IndexletManagerTest.cc:671-679", entries=[EARTH],
         queries=[q("air", "air", [])]),
    dict(name="lookupIndexKeys_single/one", lines="src/IndexletManagerTest.cc:681-703", entries=[AIR],
         queries=[q("air", "air", [5678]), q("a", "c", [5678])]),
    dict(name="lookupIndexKeys_single/two", lines="src/IndexletManagerTest.cc:706-717", entries=[AIR, EARTH],
         queries=[q("a", "c", [5678])]),
    dict(name="lookupIndexKeys_multiple", lines="src/IndexletManagerTest.cc:719-776", entries=[AIR, EARTH, FIRE],
         queries=[q("air", "air", [5678]), q("earth", "earth", [9876]), q("fire", "fire", [5432]),
                  q("air", "fire", [5678, 9876, 5432]), q("a", "g", [5678, 9876, 5432])]),
    dict(name="lookupIndexKeys_duplicate", lines="src/IndexletManagerTest.cc:778-791",
         entries=[dict(key="air", hash=1234), dict(key="air", hash=5678)],
         queries=[q("air", "air", [1234, 5678])]),
    dict(name="lookupIndexKeys_firstAllowedKeyHash", lines="src/IndexletManagerTest.cc:793-820",
         entries=[dict(key="air", hash=1234), dict(key="air", hash=5678), dict(key="air", hash=9012)],
         queries=[q("air", "air", [5678, 9012], fah=2000), q("air", "air", [5678, 9012], fah=5678)]),
    dict(name="lookupIndexKeys_largerThanMax", lines="src/IndexletManagerTest.cc:842-867", entries=[AIR, EARTH, FIRE],
         queries=[q("a", "g", [5678, 9876], mx=2, next_key_length=4, next_key="fire", next_key_hash=5432)]),
]

# keyCompare(a, b): -1 below, 0 equal, 1 above
KEY_COMPARE = [dict(a="abc", b="abc", sign=0), dict(a="abb", b="abc", sign=-1), dict(a="abd", b="abc", sign=1),
               dict(a="ab", b="abc", sign=-1), dict(a="abcd", b="abc", sign=1), dict(a="abbc", b="abc", sign=-1),
               dict(a="ac", b="abc", sign=1), dict(a="", b="abc", sign=-1), dict(a="abc", b="", sign=-1),
               dict(a="", b="", sign=-1)]


def main():
    ref = {"source": "src/IndexletManagerTest.cc:661-867 (lookupIndexKeys), src/IndexKeyTest.cc:29-41 (keyCompare)",
           "table_id": 1, "index_id": 1, "scenarios": SCENARIOS, "key_compare": KEY_COMPARE}
    out = os.path.join(HERE, "index_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(SCENARIOS), "scenarios,", len(KEY_COMPARE), "pairs")


if __name__ == "__main__":
    main()
