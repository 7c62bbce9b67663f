"""ramcrc_replay_resolve_host: which replayed objects and tombstones a recovery
master keeps (ObjectManager::replaySegment, src/ObjectManager.cc:632-867), on
the host.  The record tables come from the oracle's checkMetadataIntegrity
restatement; the expected winners from resolve_cases.replay (a plain-Python
sequential replay with a dict for the hash table) and, for the reference's own
test cases, from tests/golden/replay_resolve_ref.json.  The device tests
(test_gpu_replay_resolve.py) run the same cases."""
import numpy as np
import pytest

from ramcloud_amd import segments

import partition_cases as pc
import resolve_cases as rc

KiB = 1024
MiB = 1 << 20


@pytest.fixture(scope="module")
def ref():
    return pc.load("replay_resolve_ref.json")


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    return rc.host_source(oracle_mod, rc.mixed_lists(), rc.MIXED_CAP, bad=[rc.MIXED_BAD])


def _one(ramcrc, oracle, entries, cap=64 * KiB, hashes=None, what=""):
    buf, certs, status, table = rc.host_source(oracle, [entries], cap)
    h = None if hashes is None else np.full(table.shape[0], hashes, np.uint64)
    return table, rc.check_host(ramcrc, buf, cap, status, table, h, what)


def test_dtypes_match_the_abi():
    assert segments.RESOLVE_COUNTS_DTYPE.itemsize == 48 and segments.RESOLVE_NONE == 0xFFFFFFFF
    assert segments.RESOLVE_COUNTS_DTYPE.names == ("objects", "tombstones", "live_objects",
                                                   "live_tombstones", "malformed", "safe_version")


def test_replay_is_order_independent(oracle_mod, mixed):
    """The claim of include/ramcrc.h, checked and not assumed: replaying a
    table's participants in any order leaves the same (version, type) per key.
    Five shuffles of each of three random cases."""
    cases = [mixed[:1] + (rc.MIXED_CAP,) + mixed[2:]]
    for seed in (21, 22):
        b, _, s, t = rc.host_source(oracle_mod, rc.mixed_lists(seed, nkeys=60, nseg=2), rc.MIXED_CAP)
        cases.append((b, rc.MIXED_CAP, s, t))
    for k, (buf, cap, status, table) in enumerate(cases):
        parts = rc.participants(buf, cap, table, status)
        want = {key: v[:2] for key, v in rc.replay(parts).items()}
        assert len(want) > 50
        rng = np.random.default_rng(100 + k)
        for _ in range(5):
            got = rc.replay(parts, rng.permutation(len(parts)).tolist())
            assert {key: v[:2] for key, v in got.items()} == want


def test_reference_scenarios(ramcrc, oracle_mod, ref):
    es, first = rc.reference_case(ref)
    table, (winner, live, counts) = _one(ramcrc, oracle_mod, es, what="reference")
    assert len(ref["cases"]) == 11
    for c, at in zip(ref["cases"], first):
        n, sv = len(c["records"]), c["survivor"]
        assert winner[at:at + n].tolist() == [at + sv["index"]] * n, c["name"]
        hdr = int(table[at + sv["index"], 3]) & 0x3F
        assert hdr == (rc.OBJ if sv["type"] == "OBJ" else rc.OBJTOMB), c["name"]
        assert c["records"][sv["index"]][2] == sv["version"]
    assert counts["live_objects"] + counts["live_tombstones"] == 11 == live.shape[0]


def test_mixed(ramcrc, mixed):
    buf, certs, status, table = mixed
    assert status[rc.MIXED_BAD, 0] & segments.SEG_OK == 0 and (status[:rc.MIXED_BAD, 0] == 1).all()
    assert rc.key_residues(buf, rc.MIXED_CAP, table, status) == set(range(16))
    winner, live, counts = rc.check_host(ramcrc, buf, rc.MIXED_CAP, status, table, what="mixed")
    assert counts["safe_version"] == 1 << 40 and counts["malformed"] >= 1
    assert counts["objects"] > 300 and counts["tombstones"] > 200
    assert counts["live_objects"] > 20 and counts["live_tombstones"] > 20
    bad = table[:, 0] == rc.MIXED_BAD
    assert bad.any() and (winner[bad] == rc.NONE).all()
    # ties of every kind occur: equal objects, equal tombstones, a tombstone over an object
    parts = rc.participants(buf, rc.MIXED_CAP, table, status)
    kinds = set()
    for w in np.unique(winner[winner != rc.NONE]):
        same = [parts[i][1] for i in np.flatnonzero(winner == w) if parts[i][3] == parts[w][3]]
        kinds.add((parts[w][1], same.count(rc.OBJ) > (parts[w][1] == rc.OBJ),
                   same.count(rc.OBJTOMB) > (parts[w][1] == rc.OBJTOMB)))
    assert {(rc.OBJ, True, False), (rc.OBJTOMB, False, True), (rc.OBJTOMB, True, False)} <= kinds


def test_collisions_with_equal_hashes(ramcrc, oracle_mod):
    table, (winner, live, counts) = _one(ramcrc, oracle_mod, rc.collision_entries(), hashes=7,
                                         what="hash 7")
    assert counts["objects"] + counts["tombstones"] == 300
    assert counts["live_objects"] + counts["live_tombstones"] == 50


def test_collisions_of_the_seed(ramcrc, oracle_mod):
    table, (winner, live, counts) = _one(ramcrc, oracle_mod, rc.seed_collision_entries(), what="seed")
    # per key bytes: table 1 keeps its version-3 tombstone, table 2^32 + 1 its version-2 object
    assert live[:, 0].tolist() == [2, 4, 6, 8, 10, 12]
    assert counts["live_objects"] == 3 and counts["live_tombstones"] == 3


def test_caller_hashes_split_keys(ramcrc, oracle_mod):
    """Equal keys with different caller hashes are different keys."""
    buf, certs, status, table = rc.host_source(oracle_mod, [rc.tiny_entries()], 64 * KiB)
    winner, live, counts = rc.check_host(ramcrc, buf, 64 * KiB, status, table,
                                         np.array([1, 2, 3], np.uint64), "split")
    assert winner.tolist() == [0, 1, 2]
    winner, _, _ = rc.check_host(ramcrc, buf, 64 * KiB, status, table, what="joined")
    assert winner.tolist() == [1, 1, 2]


def test_wide_versions(ramcrc, oracle_mod):
    table, (winner, live, counts) = _one(ramcrc, oracle_mod, rc.wide_version_entries(), what="wide")
    n = 0
    for a in rc.WIDE:
        for b in rc.WIDE:
            at = 1 + 4 * n
            assert winner[at] == winner[at + 1] == (at + 1 if b > a else at), (a, b)
            assert winner[at + 2] == winner[at + 3] == (at + 3 if b > a else at + 2), (a, b)
            n += 1


@pytest.mark.parametrize("tombstones", [True, False])
def test_one_hot_key(ramcrc, oracle_mod, tombstones):
    table, (winner, live, counts) = _one(ramcrc, oracle_mod, rc.hot_key_entries(tombstones),
                                         cap=1 * MiB, what="hot")
    assert table.shape[0] == 20000
    assert (winner == (19990 if tombstones else 0)).all() and live.tolist() == [[winner[0], 0]]


def test_list_capacity(ramcrc, mixed):
    buf, certs, status, table = mixed
    _, e_live, _ = rc.expected(buf, rc.MIXED_CAP, table, status)
    need = e_live.shape[0]
    for cap in (need - 1, 0):
        winner, live, got, counts = ramcrc.replay_resolve_host(buf, rc.MIXED_CAP, 4, status, table,
                                                               live_cap=cap)
        assert got == need and np.array_equal(live, e_live[:cap])
        assert counts["live_objects"] + counts["live_tombstones"] == need


def test_refusal(ramcrc, mixed):
    buf, certs, status, table = mixed
    t = table.copy()
    t[5, 0] = 4
    with pytest.raises(ramcrc.RamcrcError) as e:
        ramcrc.replay_resolve_host(buf, rc.MIXED_CAP, 4, status, t)
    assert e.value.code == ramcrc.EINVAL
    rc.check_host(ramcrc, buf, rc.MIXED_CAP, status, table, what="after the refusal")


def test_empty_inputs(ramcrc, oracle_mod):
    buf, certs, status, table = rc.host_source(
        oracle_mod, [[pc.entry(pc.SEGHEADER, pc.seg_header(1)), pc.entry(pc.LOGDIGEST, b"d")]], 64 * KiB)
    winner, live, counts = rc.check_host(ramcrc, buf, 64 * KiB, status, table, what="no participants")
    assert (winner == rc.NONE).all() and live.shape[0] == 0 and not any(counts.values())
    winner, live, need, counts = ramcrc.replay_resolve_host(buf, 64 * KiB, 1, status, table[:0])
    assert winner.size == 0 and need == 0 and not any(rc.counts_dict(counts).values())
