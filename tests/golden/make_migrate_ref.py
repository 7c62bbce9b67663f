"""Writes tests/golden/migrate_ref.json: what the reference's own tests state
about a tablet migration's source side, restated in our words.

  MasterServiceTest.migrateSingleLogEntry_basic (src/MasterServiceTest.cc:867-900):
      key "1" of table 1 with the value "value"; table 1, the whole hash range
      -> 1 object, totalBytes 33 (the object's payload: a 24-byte header, the
      key count, one cumulative key length, 1 key byte, 5 value bytes).
  _wrongTable (:902-936): the same object asked for as table 2 -> nothing.
  _wrongKeyHash (:938-972): the same object, hash range [0, 0] -> nothing.
  migrateTablet_movingData (:1318-1362): key "hi", value "abcdefg" of table 1,
      the whole range -> "sent 1 objects and 0 tombstones ... 92 bytes in
      total".  The 92 bytes are the object's 36 and a 56-byte RPCRESULT record
      of the write (a 44-byte header and the 12-byte write response).  Our call
      leaves that record with the master: the fixture pins 1 object, 0
      tombstones and 36 payload bytes, and records the RPCRESULT as one skipped
      record of 56 bytes.

    python tests/golden/make_migrate_ref.py
"""
import json
import os

ALL = (1 << 64) - 1


def obj(key, value):
    return dict(type="OBJ", table_id=1, key=key, value=value, version=1)


def main():
    one = [obj("1", "value")]
    cases = [
        dict(name="migrateSingleLogEntry_basic", records=one, table_id=1, first_hash=0, last_hash=ALL,
             expect=dict(objects=1, tombstones=0, payload_bytes=33, skipped_other=0, skipped_other_bytes=0)),
        dict(name="migrateSingleLogEntry_wrongTable", records=one, table_id=2, first_hash=0, last_hash=ALL,
             expect=dict(objects=0, tombstones=0, payload_bytes=0, skipped_other=0, skipped_other_bytes=0)),
        dict(name="migrateSingleLogEntry_wrongKeyHash", records=one, table_id=1, first_hash=0, last_hash=0,
             expect=dict(objects=0, tombstones=0, payload_bytes=0, skipped_other=0, skipped_other_bytes=0)),
        dict(name="migrateTablet_movingData",
             records=[obj("hi", "abcdefg"),
                      dict(type="RPCRESULT", table_id=1, response_bytes=12, payload_bytes=56)],
             table_id=1, first_hash=0, last_hash=ALL, reference_total_bytes=92,
             expect=dict(objects=1, tombstones=0, payload_bytes=36, skipped_other=1, skipped_other_bytes=56)),
    ]
    out = dict(source="src/MasterServiceTest.cc:867-972, :1318-1362", cases=cases)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "migrate_ref.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
