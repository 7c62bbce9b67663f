"""ramcrc_recovery_partition_host: the placement decision of
RecoverySegmentBuilder::build (src/RecoverySegmentBuilder.cc:74-201) on the
host -- key hash, tablet lookup, liveness.  The record tables come from the
oracle's checkMetadataIntegrity restatement; the expected lists from
partition_cases.expected (plain Python) and, where they hold the answer, from
the fixtures tests/golden/key_hash_ref.json and recovery_build_ref.json."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import partition_cases as pc

KiB = 1024
ALL = (1 << 64) - 1
OK, MAL = segments.SEG_OK, segments.SEG_MALFORMED


@pytest.fixture(scope="module")
def hash_ref():
    return pc.load("key_hash_ref.json")["cases"]


@pytest.fixture(scope="module")
def build_ref():
    return pc.load("recovery_build_ref.json")


def _one(ramcrc, oracle, entries, tabs, n_part, cap=64 * KiB, what=""):
    buf, certs, status, table = pc.host_source(oracle, [entries], cap)
    place, hashes, pstat = pc.check_host(ramcrc, buf, cap, status, table, tabs, n_part, what)
    return table, place, hashes, pstat


def test_dtypes_match_the_abi():
    assert segments.TABLET_DTYPE.itemsize == 40 and segments.PARTITION_STATUS_DTYPE.itemsize == 16
    assert segments.SEG_NO_HEADER == 512 and segments.SEG_MALFORMED == 1024
    taken = (segments.SEG_OK | segments.SEG_PAST_CAPACITY | segments.SEG_PAST_LENGTH
             | segments.SEG_BAD_CHECKSUM | segments.SEG_TABLE_FULL | segments.SEG_CYCLE
             | segments.SEG_APPEND_FULL | segments.SEG_SOURCE_BAD | 0x100)
    assert not (segments.SEG_NO_HEADER | segments.SEG_MALFORMED) & taken


def test_restatement_matches_the_fixture(hash_ref):
    for t, key, h in hash_ref:
        assert pc.key_hash(t, bytes.fromhex(key)) == h


def test_key_hash_fixture(ramcrc, oracle_mod, hash_ref):
    """Every key_hash_ref.json case as an object or a tombstone (alternating)."""
    cap = 512 * KiB
    es = [pc.entry(pc.SEGHEADER, pc.seg_header(1))]
    for i, (t, key, _) in enumerate(hash_ref):
        key = bytes.fromhex(key)
        es.append(pc.entry(pc.OBJ, pc.obj(t, key, b"v" * (i % 7))) if i % 2 == 0
                  else pc.entry(pc.OBJTOMB, pc.tomb(t, key)))
    buf, certs, status, table = pc.host_source(oracle_mod, [es], cap)
    _, _, hashes, pstat = ramcrc.recovery_partition_host(buf, cap, 1, status, table,
                                                         pc.tablets([]), 1)
    assert hashes[0] == 0
    assert hashes[1:].tolist() == [h for _, _, h in hash_ref]
    assert pstat.tolist() == [[OK, 0, len(hash_ref), 0]]


def _scenario(build_ref, sc):
    return [pc.entry(t, bytes.fromhex(p)) for t, p in sc["entries"]], pc.tablets(build_ref["tablets"])


@pytest.mark.parametrize("which", [0, 1, 2])
def test_build_scenarios(ramcrc, oracle_mod, build_ref, which):
    """RecoverySegmentBuilderTest's build, build_safeVersionEntries and
    build_participantList: partition, then ramcrc_recovery_append_host; every
    output's (type, offset, length) sequence is the fixture's, every
    certificate the oracle's."""
    sc = build_ref["scenarios"][which]
    es, tabs = _scenario(build_ref, sc)
    cap, n_part = 64 * KiB, sc["n_part"]
    buf, certs, status, table = pc.host_source(oracle_mod, [es], cap)
    place, _, pstat = pc.check_host(ramcrc, buf, cap, status, table, tabs, n_part, sc["name"])
    out = np.full(n_part * cap, ac.FILL, np.uint8)
    got_certs, got_stat = ramcrc.recovery_append_host(buf, cap, 1, status, table, place, n_part, out,
                                                      cap, cap)
    exp = ac.expected(buf, cap, table, status, place, 1, n_part, cap)
    ac.check_outputs(oracle_mod, exp, out, cap, cap, got_certs, got_stat, sc["name"])
    for p in range(n_part):
        region = out[p * cap:(p + 1) * cap]
        assert pc.walk_records(region, int(got_certs[p, 0])) == sc["outputs"][p], (sc["name"], p)
    assert pstat[0, 0] == OK and pstat[0, 1] == sum(len(o) for o in sc["outputs"])
    if "object_keys" in sc:
        assert pstat[0].tolist()[2:] == [sc["unplaced"], sc["dead"]]
        for p, key in enumerate(sc["object_keys"]):   # the object's key is its payload byte 27
            assert bytes(out[p * cap + 14 + 2 + 27:p * cap + 14 + 2 + 28]).decode() == key


def test_is_entry_alive(ramcrc, oracle_mod, build_ref):
    ref = build_ref["is_entry_alive"]
    cid, coff = ref["ctime"]
    for seg_id, off, alive in ref["cases"]:
        # a SEGHEADER naming seg_id, padding, then a tombstone at byte `off`
        hdr = pc.entry(pc.SEGHEADER, pc.seg_header(seg_id))
        pad = pc.entry(pc.LOGDIGEST, b"\0" * (off - len(hdr) - 3))
        assert len(hdr) + len(pad) == off
        es = [hdr, pad, pc.entry(pc.OBJTOMB, pc.tomb(2, b"1"))]
        table, place, _, pstat = _one(ramcrc, oracle_mod, es, [(2, 0, ALL, cid, coff, 0)], 1,
                                      what=(seg_id, off))
        assert table[2, 1] == off
        assert place.tolist() == ([[2, 0]] if alive else [])
        assert pstat.tolist() == [[OK, int(alive), 0, int(not alive)]]


def test_which_partition(ramcrc, oracle_mod, build_ref):
    tabs = pc.tablets(build_ref["tablets"])
    tabs["ctime_segment_id"] = 0
    for t, key, part in build_ref["which_partition"]:
        es = pc.head_entries()[:1] + [pc.entry(pc.OBJ, pc.obj(t, key.encode(), b"v"))]
        _, place, _, pstat = _one(ramcrc, oracle_mod, es, tabs, 2, what=(t, key))
        if part is None:
            assert place.shape[0] == 0 and pstat[0, 2] == 1
        else:
            assert place.shape[0] == 1 and place[0, 0] == 1 and (part < 0 or place[0, 1] == part)


def test_types(ramcrc, oracle_mod):
    """Every type's fields; types build skips; empty keys; the stored hashes."""
    h = pc.key_hash
    tabs = [(7, 0, ALL, 0, 0, 2), (1 << 40, 0, ALL, 0, 0, 1)]
    es = pc.head_entries(5) + [
        pc.entry(pc.OBJ, pc.obj(7, b"key", b"value")),
        pc.entry(pc.OBJ, pc.obj(7, b"", b"value", num_keys=0)),        # no key: the empty key
        pc.entry(pc.OBJ, pc.obj(7, b"", b"value")),                    # key length 0
        pc.entry(pc.OBJ, pc.obj(7, b"abcdefg", b"v", num_keys=3)),     # the first of three keys
        pc.entry(pc.PREP, pc.prep(7, b"prepared", b"x" * 300)),
        pc.entry(pc.OBJTOMB, pc.tomb(7, b"")),
        pc.entry(pc.OBJTOMB, pc.tomb(1 << 40, b"tombstone key")),
        pc.entry(pc.RPCRESULT, pc.rpc_result(7, 11, response=b"resp")),
        pc.entry(pc.PREPTOMB, pc.prep_tomb(7, 12)),
        pc.entry(pc.TXDECISION, pc.tx_decision(1 << 40, ALL)),
        pc.entry(6, b"table stats"), pc.entry(0, b""), pc.entry(12, b"unknown"), pc.entry(63, b"x" * 70),
        pc.entry(pc.SEGHEADER, pc.seg_header(5)),
    ]
    table, place, hashes, pstat = _one(ramcrc, oracle_mod, es, tabs, 3)
    assert hashes[3:13].tolist() == [h(7, b"key"), h(7, b""), h(7, b""), h(7, b"abcdefg"),
                                     h(7, b"prepared"), h(7, b""), h(1 << 40, b"tombstone key"),
                                     11, 12, ALL]
    assert place.tolist() == [[2, 0], [2, 1], [2, 2]] + [[r, 2] for r in range(3, 9)] + [
        [9, 1], [10, 2], [11, 2], [12, 1]]
    assert pstat.tolist() == [[OK, 13, 0, 0]]


def test_tablet_lookup(ramcrc, oracle_mod):
    """Inclusive bounds, unsigned compare, the first of overlapping tablets,
    the full table id, no tablets at all."""
    es, base, overlap = pc.stored_entries(), pc.TAB_BASE, pc.TAB_OVERLAP
    for tabs in (base, base + overlap, overlap[::-1] + base, [], base[:1]):
        _, place, _, _ = _one(ramcrc, oracle_mod, es, tabs, 7, what=len(tabs))
        got = dict(place[7:].tolist())   # (behind the safe version's 7 placements)
        if tabs == base:
            assert got == pc.TAB_BASE_PLACED
        if tabs and tabs[0] == overlap[1]:
            assert got[3 + 4] == 6 and got[3 + 0] == 5


def test_fan_out(ramcrc, oracle_mod):
    """Safe versions go everywhere; a participant list to the owners of its
    participants, in participant order, repeats included."""
    for n_part in (3, 64, 600):
        es, tabs, body = pc.fan_out_case(n_part)
        _, place, _, pstat = _one(ramcrc, oracle_mod, es, tabs, n_part)
        assert place[n_part:-n_part].tolist() == body
        assert place[-n_part:].tolist() == [[9, p] for p in range(n_part)]
        assert pstat.tolist() == [[OK, 2 * n_part + 74, 0, 0]]


def test_malformed(ramcrc, oracle_mod):
    """Records too short for their fields are left out, counted nowhere, and
    flag the segment; the same records one byte longer are placed."""
    key = b"0123456789"
    o, p = pc.obj(1, key), pc.prep(1, key)
    short = [(pc.OBJ, o[:24]), (pc.OBJ, o[:26]), (pc.OBJ, o[:-1]), (pc.PREP, p[:56]), (pc.PREP, p[:58]),
             (pc.PREP, p[:-1]), (pc.OBJTOMB, pc.tomb(1, b"")[:31]), (pc.RPCRESULT, b"\1" * 15),
             (pc.PREPTOMB, b"\1" * 15), (pc.TXDECISION, b""), (pc.TXPLIST, pc.tx_plist([])[:23]),
             (pc.TXPLIST, pc.tx_plist([(1, 1, 1)] * 3)[:-1]), (pc.TXPLIST, pc.tx_plist([], count=1 << 31)),
             (pc.OBJ, pc.obj(1, key, num_keys=200, key_len=10)[:300])]
    good = [(pc.OBJ, o), (pc.OBJ, pc.obj(1, b"", num_keys=0)[:25]), (pc.PREP, p),
            (pc.OBJTOMB, pc.tomb(1, b"")), (pc.RPCRESULT, b"\1" * 16), (pc.TXPLIST, pc.tx_plist([])),
            (pc.SAFEVERSION, b"")]
    tabs = [(1, 0, ALL, 0, 0, 0), (0x0101010101010101, 0, ALL, 0, 0, 0)]
    es = pc.head_entries() + [pc.entry(t, b) for t, b in short + good]
    table, place, hashes, pstat = _one(ramcrc, oracle_mod, es, tabs, 1)
    n0 = 3 + len(short)
    assert place[:, 0].tolist() == [2] + [n0 + k for k in (0, 1, 2, 3, 4, 6)]
    assert (hashes[3:n0] == 0).all()
    assert pstat.tolist() == [[OK | MAL, 7, 0, 0]]
    # a hand-edited table: OVERLONG, and a payload past the stride
    for damage in ("overlong_flag", "payload_past_stride"):
        buf, certs, status, table = pc.host_source(oracle_mod, [es], 64 * KiB)
        ac.damage_record(table, n0, damage, 64 * KiB)
        place, _, pstat = pc.check_host(ramcrc, buf, 64 * KiB, status, table, pc.tablets(tabs), 1, damage)
        assert n0 not in place[:, 0].tolist() and pstat[0, 1] == 6


def test_segments_that_place_nothing(ramcrc, oracle_mod):
    """A source that failed its check; a placed record before any SEGHEADER; a
    19-byte SEGHEADER; a second SEGHEADER in mid-segment changes the position;
    records build skips need no header."""
    cap, lists = 64 * KiB, pc.position_lists()
    buf, certs = ac.source_of(oracle_mod, lists, cap)
    certs[1, 1] ^= 1
    status, table = ac.host_walk(oracle_mod, buf, certs, len(lists), cap)
    place, _, pstat = pc.check_host(ramcrc, buf, cap, status, table, [(1, 0, ALL, 7, 0, 1)], 2)
    assert pstat.tolist() == pc.POSITION_STATUS
    assert sorted(set(table[place[:, 0], 0].tolist())) == [0, 4, 5]


def test_place_cap(ramcrc, oracle_mod):
    """A list longer than place_cap: the needed count comes back, nothing is
    written past the capacity."""
    es = pc.head_entries() + [pc.entry(pc.OBJTOMB, pc.tomb(1, bytes([k]))) for k in range(50)]
    buf, certs, status, table = pc.host_source(oracle_mod, [es], 64 * KiB)
    tabs = pc.tablets([(1, 0, ALL, 0, 0, 1)])
    full, need, _, _ = ramcrc.recovery_partition_host(buf, 64 * KiB, 1, status, table, tabs, 2)
    assert need == 52 and full.shape[0] == 52
    for cap in (52, 51, 1, 0):
        place, need, _, pstat = ramcrc.recovery_partition_host(buf, 64 * KiB, 1, status, table, tabs, 2,
                                                               place_cap=cap)
        assert need == 52 and np.array_equal(place, full[:cap]) and pstat[0, 1] == 52


@pytest.mark.parametrize("variant", ["partition_at_n_part", "n_part_zero", "segment_at_n_seg",
                                     "second_run"])
def test_refusals(ramcrc, oracle_mod, variant):
    cap = 64 * KiB
    lists = [pc.head_entries() + [pc.entry(pc.OBJTOMB, pc.tomb(1, b"k"))] for _ in range(2)]
    buf, certs = ac.source_of(oracle_mod, lists, cap)
    status, table = ac.host_walk(oracle_mod, buf, certs, 2, cap)
    tabs, n_part, bad = [(1, 0, ALL, 0, 0, 1)], 2, table.copy()
    if variant == "partition_at_n_part":
        tabs = tabs + [(5, 0, 0, 0, 0, 2)]
    elif variant == "n_part_zero":
        n_part, tabs = 0, []
    elif variant == "segment_at_n_seg":
        bad[-1, 0] = 2
    else:
        bad[-1, 0] = 0
    with pytest.raises(ramcrc.RamcrcError) as e:
        ramcrc.recovery_partition_host(buf, cap, 2, status, bad, pc.tablets(tabs), n_part)
    assert e.value.code == ramcrc.EINVAL
    pc.check_host(ramcrc, buf, cap, status, table, [(1, 0, ALL, 0, 0, 1)], 2)
