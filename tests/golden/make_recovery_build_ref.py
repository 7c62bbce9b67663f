"""Generate tests/golden/recovery_build_ref.json (run in the build container only).

The scenarios of the reference's RecoverySegmentBuilderTest as data:
  * src/RecoverySegmentBuilderTest.cc:41-65: the four tablets;
  * :70-275 (build), :277-304 (build_safeVersionEntries), :306-334
    (build_participantList): the records appended to a head segment, and per
    recovery segment the (type, offset, length) sequence that the test's
    expected dumpSegment strings state;
  * :370-392: the five isEntryAlive cases; :394-407: the four whichPartition
    cases.

A head segment opens with a SEGHEADER, a log digest and safe version 1, which
is why every expected output starts with "safeVersion at offset 0, length 12".
The records are built by tests/partition_cases.py (our own restatement of the
layouts, checksum fields zero); nothing is compiled or copied from the
reference.  The key hashes the test's strings print, 0xDD5D9F7F60D5B056 for
(1, "1") and 0x3554F985FBED3C16 for (1, "2"), are asserted before anything is
written.

Usage:  python tests/golden/make_recovery_build_ref.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import partition_cases as pc  # noqa: E402

ALL = (1 << 64) - 1


def main():
    h = {(t, k): pc.key_hash(t, k) for t in (1, 2, 3, 10) for k in (b"1", b"2")}
    assert h[1, b"1"] == 0xDD5D9F7F60D5B056 and h[1, b"2"] == 0x3554F985FBED3C16
    # (table id, start, end, ctime segment id, ctime offset, partition), :56-60
    tablets = [[1, 0, h[1, b"1"] - 1, 0, 0, 0], [1, h[1, b"1"], ALL, 0, 0, 1],
               [2, 0, ALL, 2, 0, 0], [3, 0, 1, 0, 0, 0]]
    E = lambda etype, payload: [etype, payload.hex()]
    head = [[int(e[0]) & 0x3F, e[2:].hex()] for e in pc.head_entries(segment_id=0)]

    build = list(head)
    for tid, key, val in ((1, b"1", b"hello\0"), (1, b"2", b"abcde\0")):    # :74-98
        build += [E(pc.OBJ, pc.obj(tid, key, val)), E(pc.OBJTOMB, pc.tomb(tid, key))]
    build += [E(pc.OBJ, pc.obj(10, b"1", b"abcde\0")), E(pc.OBJ, pc.obj(2, b"1", b"abcde\0"))]
    for tid, key, lease, rpc, ack in ((1, b"1", 6, 4, 2), (1, b"2", 5, 3, 1), (10, b"1", 10, 5, 2),
                                      (2, b"1", 2, 1, 0)):                 # :115-142
        build.append(E(pc.RPCRESULT, pc.rpc_result(tid, h[tid, key], lease, rpc, ack)))
    for tid, key in ((1, b"1"), (1, b"2"), (10, b"1"), (2, b"1")):         # :143-203
        build += [E(pc.PREP, pc.prep(tid, key, b"hello\0")),
                  E(pc.PREPTOMB, pc.prep_tomb(tid, h[tid, key]))]
    for tid, key, lease in ((1, b"1", 6), (1, b"2", 5), (10, b"1", 10), (2, b"1", 2)):   # :204-232
        build.append(E(pc.TXDECISION, pc.tx_decision(tid, h[tid, key], lease)))
    seq = [[pc.SAFEVERSION, 0, 12], [pc.OBJ, 14, 34], [pc.OBJTOMB, 50, 33], [pc.RPCRESULT, 85, 44],
           [pc.PREP, 131, 66], [pc.PREPTOMB, 199, 44], [pc.TXDECISION, 245, 48]]   # :246-269

    safe = head + [E(pc.SAFEVERSION, pc.safe_version(99))]                  # :281-286
    plist = head + [E(pc.TXPLIST, pc.tx_plist([(1, 2, 10), (123, 234, 11), (111, 222, 12)]))]   # :311-319

    out = {
        "_source": __doc__.strip().splitlines()[0],
        "tablets": tablets,
        "scenarios": [
            {"name": "build", "cite": "src/RecoverySegmentBuilderTest.cc:70-275", "n_part": 2,
             "entries": build, "outputs": [seq, seq],
             # which key the object of each output holds (:247, :259)
             "object_keys": ["2", "1"], "unplaced": 5, "dead": 5},   # the records of tables 10 and 2
            {"name": "build_safeVersionEntries", "cite": ":277-304", "n_part": 3, "entries": safe,
             "outputs": [[[pc.SAFEVERSION, 0, 12], [pc.SAFEVERSION, 14, 12]]] * 3},
            {"name": "build_participantList", "cite": ":306-334", "n_part": 2, "entries": plist,
             "outputs": [[[pc.SAFEVERSION, 0, 12], [pc.TXPLIST, 14, 96]], [[pc.SAFEVERSION, 0, 12]]]},
        ],
        # tablet 2's creation position set to (12741, 57273); {segment id, offset} -> alive (:370-392)
        "is_entry_alive": {"ctime": [12741, 57273],
                           "cases": [[12741, 57273, True], [12741, 57274, True], [12742, 57274, True],
                                     [12740, 57273, False], [12741, 57272, False]]},
        # (table id, key) -> partition, or null where the test expects no tablet;
        # -1: found, the test does not state which (:394-407)
        "which_partition": [[1, "1", 1], [1, "2", -1], [2, "1", 0], [3, "1", None]],
    }
    path = os.path.join(HERE, "recovery_build_ref.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in out.items())
                + "\n}\n")   # one key per line
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
