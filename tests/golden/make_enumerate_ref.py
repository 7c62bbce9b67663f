"""Generate tests/golden/enumerate_ref.json.

What the reference's own tests say about a table enumeration (ENUMERATE), as
data in our own words:

  - MasterServiceTest.enumerate_basics (src/MasterServiceTest.cc:510-556): two
    one-key objects in table 1, keys "0" and "1", 6-byte values; it expects a
    payload of 76 bytes, two entries of length 34 (at 0 and at 38), and 0
    bytes from a second call that starts at the returned cursor;
  - MasterServiceTest.enumerate_mergeTablet (:568-620): keys "012345" and
    "678910" of table 1, whose hashes the test states as
    0x7fc19e9dda158f61 and 0xb1e38b2242e1bbf4; a stale frame over [0,
    0x8fffffffffffffff] that stands at bucket num_buckets * 4 / 5, hash 0; it
    expects one entry, length 39, payload 43, key "678910": the other key's
    bucket lies below 4/5 of the old table.  The test takes num_buckets from
    its hash table; 2^16 stands for it here, at which the first hash's bucket,
    36705, is below 52428 and so hidden;
  - TableEnumeratorTest.keysOnly (src/TableEnumeratorTest.cc:168-251): five
    one-key objects "0" .. "4" of one table with 6-byte values, enumerated
    with keysOnly; it expects five entries of 28 bytes with value length 0.
    The order it sees is its bucket layout's and is not pinned here: the set
    of keys is.  (Its table id comes from createTable; 1 stands for it.)

The length of an entry is that of the object's log entry: the 24-byte header,
the key count, one cumulative length per key, the keys, the value; with keys
only it ends before the value.  Nothing is compiled or copied from the
reference; the project's plain-Python Key::getHash (tests/partition_cases.py)
is asserted to give both stated constants before anything is written.

Usage:  python tests/golden/make_enumerate_ref.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import partition_cases as pc  # noqa: E402

# an object's log entry: header, key count, cumulative lengths, the keys, the value
entry = lambda keys, value: 24 + 1 + 2 * len(keys) + sum(len(k) for k in keys) + len(value)

FRAME_BUCKETS = 1 << 16

SCENARIOS = [
    dict(name="MasterServiceTest.enumerate_basics", lines="src/MasterServiceTest.cc:510-556", table_id=1,
         objects=[dict(key="0", value="abcdef"), dict(key="1", value="ghijkl")], keys_only=False, stale=[],
         entry_lengths=[34, 34], payload_bytes=76, returned_keys=["0", "1"], order_pinned=False,
         second_call_bytes=0),
    dict(name="MasterServiceTest.enumerate_mergeTablet", lines="src/MasterServiceTest.cc:568-620", table_id=1,
         objects=[dict(key="012345", value="abcdef"), dict(key="678910", value="ghijkl")], keys_only=False,
         stale=[dict(tablet_start_hash=0, tablet_end_hash=0x8fffffffffffffff, num_buckets=FRAME_BUCKETS,
                     bucket_index=FRAME_BUCKETS * 4 // 5, bucket_next_hash=0)],
         entry_lengths=[39], payload_bytes=43, returned_keys=["678910"], order_pinned=True,
         second_call_bytes=0),
    dict(name="TableEnumeratorTest.keysOnly", lines="src/TableEnumeratorTest.cc:168-251", table_id=1,
         objects=[dict(key="0", value="abcdef"), dict(key="1", value="ghijkl"), dict(key="2", value="mnopqr"),
                  dict(key="3", value="stuvwx"), dict(key="4", value="yzabcd")], keys_only=True, stale=[],
         entry_lengths=[28] * 5, payload_bytes=5 * 32, returned_keys=["0", "1", "2", "3", "4"],
         order_pinned=False, second_call_bytes=0),
]

CONSTANTS = [dict(table_id=1, key="012345", hash=0x7fc19e9dda158f61),
             dict(table_id=1, key="678910", hash=0xb1e38b2242e1bbf4)]


def main():
    for c in CONSTANTS:
        assert pc.key_hash(c["table_id"], c["key"].encode()) == c["hash"], c
    assert entry(["0"], "abcdef") == 34 and entry(["012345"], "ghijkl") == 39 and entry(["0"], "") == 28
    low48 = lambda h: h & 0xffffffffffff
    assert low48(CONSTANTS[0]["hash"]) & (FRAME_BUCKETS - 1) == 36705 < FRAME_BUCKETS * 4 // 5 == 52428
    assert low48(CONSTANTS[1]["hash"]) & (FRAME_BUCKETS - 1) == 0xbbf4   # 48116 < 52428, but
    assert CONSTANTS[1]["hash"] > 0x8fffffffffffffff                     # outside the stale frame's tablet
    ref = {"source": "src/MasterServiceTest.cc:510-556, :568-620 (enumerate), "
                     "src/TableEnumeratorTest.cc:168-251 (keysOnly)",
           "entry": {"length_bytes": 4, "object_header_bytes": 24},
           "key_hash_constants": CONSTANTS, "scenarios": SCENARIOS}
    out = os.path.join(HERE, "enumerate_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(SCENARIOS), "scenarios")


if __name__ == "__main__":
    main()
