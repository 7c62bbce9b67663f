"""Generate tests/golden/multi_read_ref.json.

What the reference's own tests say about a multi-read, as data in our own
words:

  - every (rules, version) -> status line of ObjectManagerTest.rejectOperation
    (src/ObjectManagerTest.cc:2388-2431);
  - the scenarios multiRead_basics, multiRead_noSuchObject and
    multiRead_bufferSizeExceeded of src/MasterServiceTest.cc:1430-1517: the
    objects the test writes (a table's first write gets version 1, the next
    2), the keys it asks for, and what its EXPECT lines find.  The last one
    sets maxResponseRpcLen = 78 and gets exactly one of two objects with a
    1-byte key and a 50-byte value: 8 bytes of MultiOp::Response, a 16-byte
    ReadPart and 54 bytes of keys and value.  Our reply_cap leaves the 8 out:
    70 returns one part and 69 none.

Nothing is compiled or copied from the reference; the plain-Python status
rule of tests/read_cases.py is asserted to agree before anything is written.

Usage:  python tests/golden/make_multi_read_ref.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import read_cases as rd  # noqa: E402

OK, DOESNT_EXIST, EXISTS, WRONG_VERSION = 0, 3, 4, 5
G = 0x400000001

# (source lines, rules, version, status)
REJECT = [
    ("2392-2396", dict(doesnt_exist=1), 0, DOESNT_EXIST),
    ("2398-2402", dict(exists=1, version_le_given=1, version_ne_given=1), 0, OK),
    ("2404-2408", dict(exists=1), 2, EXISTS),
    ("2410-2415", dict(given_version=G, version_le_given=1), G - 1, WRONG_VERSION),
    ("2416-2417", dict(given_version=G, version_le_given=1), G, WRONG_VERSION),
    ("2418-2419", dict(given_version=G, version_le_given=1), G + 1, OK),
    ("2421-2426", dict(given_version=G, version_ne_given=1), G - 1, WRONG_VERSION),
    ("2427-2428", dict(given_version=G, version_ne_given=1), G, OK),
    ("2429-2430", dict(given_version=G, version_ne_given=1), G + 1, WRONG_VERSION),
]

CHUNK_A = "chunk1:12 chunk2:12 chunk3:12 chunk4:12 chunk5:12 "
CHUNK_B = "chunk6:12 chunk7:12 chunk8:12 chunk9:12 chunk10:12"

# keys and value of a one-key object: key count, one cumulative length, the key, the value
kv = lambda key, value: 1 + 2 + len(key) + len(value)

SCENARIOS = [
    dict(name="multiRead_basics", lines="1430-1448", table_id=1,
         objects=[["0", "firstVal", 1], ["1", "secondVal", 2]], queries=["0", "1"],
         parts=[dict(status=OK, version=1, value="firstVal", length=kv("0", "firstVal")),
                dict(status=OK, version=2, value="secondVal", length=kv("1", "secondVal"))]),
    dict(name="multiRead_noSuchObject", lines="1509-1517", table_id=1, objects=[], queries=["bogus"],
         parts=[dict(status=DOESNT_EXIST)]),
    dict(name="multiRead_bufferSizeExceeded", lines="1450-1484", table_id=1,
         objects=[["0", CHUNK_A, 1], ["1", CHUNK_B, 2]], queries=["0", "1"], max_response_rpc_len=78,
         parts=[dict(status=OK, version=1, value=CHUNK_A, length=kv("0", CHUNK_A)),
                dict(status=OK, version=2, value=CHUNK_B, length=kv("1", CHUNK_B))],
         caps=[dict(reply_cap=78 - 8, returned=1), dict(reply_cap=78 - 8 - 1, returned=0)]),
]


def main():
    assert len(CHUNK_A) == 50 and len(CHUNK_B) == 50 and 8 + 16 + kv("0", CHUNK_A) == 78
    reject = []
    for lines, rules, version, status in REJECT:
        assert rd.reject(rules, version) == status, lines
        reject.append({"lines": lines, "rules": rules, "version": version, "status": status})
    ref = {"source": "src/ObjectManagerTest.cc:2388-2431 (rejectOperation), "
                     "src/MasterServiceTest.cc:1430-1517 (multiRead_*)",
           "reject": reject, "scenarios": SCENARIOS}
    out = os.path.join(HERE, "multi_read_ref.json")
    with open(out, "w") as f:
        json.dump(ref, f, indent=1)
        f.write("\n")
    print(out, len(reject), "reject lines,", len(SCENARIOS), "scenarios")


if __name__ == "__main__":
    main()
