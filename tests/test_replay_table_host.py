"""ramcrc_replay_table_*_host: ramcrc_replay_resolve_host's decision fed batch
by batch into a table that stays (MasterService::recover replays recovery
segments as they arrive, src/MasterService.cc:3501-3720).  The record tables
come from the oracle's checkMetadataIntegrity restatement; the expectation is
the one-call resolve over the concatenation of the added batches
(replay_table_cases.expect), mapped back to {batch, record}.  The device tests
(test_gpu_replay_table.py) run the same cases."""
import numpy as np
import pytest

from ramcloud_amd import segments

import partition_cases as pc
import replay_table_cases as tc
import resolve_cases as rc

KiB = 1024
MiB = 1 << 20


def _batches(oracle, lists_per_batch, cap=64 * KiB, bad=()):
    return [tc.HostBatch(oracle, lists, cap, bad=[0] if j in bad else [])
            for j, lists in enumerate(lists_per_batch)]


@pytest.fixture(scope="module")
def relations(ramcrc, oracle_mod):
    """(batches, expectation after 1, 2 and 3 adds): computed once, shared."""
    bs = _batches(oracle_mod, [[es] for es in tc.relation_lists()])
    return bs, [tc.expect(ramcrc, bs[:k + 1]) for k in range(3)]


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    return _batches(oracle_mod, [[es] for es in rc.mixed_lists()], rc.MIXED_CAP, bad=[rc.MIXED_BAD])


@pytest.fixture(scope="module")
def hot(oracle_mod):
    return tc.HostBatch(oracle_mod, [rc.hot_key_entries()], 1 * MiB)


def test_dtypes_match_the_abi():
    assert segments.REPLAY_REF_DTYPE.itemsize == 8 and segments.REPLAY_REF_DTYPE.names == ("batch", "record")
    assert segments.REPLAY_TABLE_STATS_DTYPE.itemsize == 48
    assert segments.REPLAY_TABLE_STATS_DTYPE.names == ("keys", "live_objects", "live_tombstones",
                                                       "safe_version", "batches", "spoiled")


# ------------------------------------------ 1. across batches, every relation
def _relations(ramcrc, relations):
    bs, exps = relations
    t = ramcrc.ReplayTableHost(2000, 3)
    got = None
    for k, b in enumerate(bs):
        assert tc.host_add(t, b) == k
        got = tc.check_host(t, exps[k], what=("after add", k))   # batch 0 after batch 2 included
    return t, got


def test_across_batches(ramcrc, relations):
    bs, exps = relations
    tc.check_relations(bs, exps[2])
    # the verdict on batch 0 changes with the later adds
    assert exps[0][0][1].shape[0] > exps[2][0][1].shape[0] > 0
    t, _ = _relations(ramcrc, relations)
    t.close()


# ----------------------------------------------------------------- 2. order
def test_order(ramcrc, mixed):
    """The four segments of the mixed case as four batches, one of them with a
    bad certificate, in five shuffled add orders: per key the surviving
    (version, type) is the sequential replay's; in the identity order every
    output is the one-call's over the four segments."""
    assert mixed[rc.MIXED_BAD].status[0, 0] & segments.SEG_OK == 0
    want = tc.replayed(mixed)
    assert len(want) > 100
    rng = np.random.default_rng(31)
    for order in [list(range(4))] + [rng.permutation(4).tolist() for _ in range(5)]:
        bs = [mixed[j] for j in order]
        t = ramcrc.ReplayTableHost(1000, 4)
        for b in bs:
            tc.host_add(t, b)
        got = tc.check_host(t, tc.expect(ramcrc, bs), what=order)
        assert tc.survivors(bs, [g[1] for g in got]) == want, order
        t.close()


# ------------------------------------------------------------ 3. collisions
def test_collisions_across_batches(ramcrc, oracle_mod):
    """Every caller hash is 7: one probe chain spans both batches, and batch
    1's records compare their keys with claimants of batch 0."""
    bs = _batches(oracle_mod, tc.split_lists(rc.collision_entries()))
    hs = [np.full(b.table.shape[0], 7, np.uint64) for b in bs]
    t = ramcrc.ReplayTableHost(64, 2)
    for b, h in zip(bs, hs):
        tc.host_add(t, b, h)
    exp = tc.expect(ramcrc, bs, hs)
    tc.check_host(t, exp, "hash 7")
    assert t.stats()["keys"] == 50 and exp[1][1].shape[0] > 0


def test_collisions_of_the_seed(ramcrc, oracle_mod):
    bs = _batches(oracle_mod, tc.split_lists(rc.seed_collision_entries(), at=6))
    t = ramcrc.ReplayTableHost(64, 2)
    for b in bs:
        tc.host_add(t, b)
    tc.check_host(t, tc.expect(ramcrc, bs), "seed")
    assert t.stats()["keys"] == 6


def test_given_and_computed_hashes_mix(ramcrc, oracle_mod, mixed):
    """The partition call's hashes for batch 0 and NULL for batch 1: identical
    to NULL for both."""
    bs = mixed[:2]
    tabs = pc.tablets([(tid, 0, tc.ALL, 0, 0, 0) for tid in (1, 2, (1 << 32) + 1)])
    _, _, h0, _ = ramcrc.recovery_partition_host(bs[0].buf, bs[0].cap, 1, bs[0].status, bs[0].table,
                                                 tabs, 1)
    exp = tc.expect(ramcrc, bs)
    for hashes in ((h0, None), (None, None)):
        t = ramcrc.ReplayTableHost(1000, 2)
        for b, h in zip(bs, hashes):
            tc.host_add(t, b, h)
        tc.check_host(t, exp, "given, then computed")
        t.close()


# ----------------------------------------------------------- 4. one hot key
def test_one_hot_key(ramcrc, hot):
    t = ramcrc.ReplayTableHost(8, 2)
    tc.host_add(t, hot)
    tc.host_add(t, hot)
    got = tc.check_host(t, tc.expect(ramcrc, [hot, hot], python=False), "hot")
    assert got[0][1].tolist() == [[19990, 0]] and got[1][1].shape[0] == 0
    assert (got[1][0]["batch"] == 0).all() and (got[1][0]["record"] == 19990).all()
    assert t.stats()["keys"] == 1


# ------------------------------------------------- 6. capacity and spoiling
def _spoiled(ramcrc, t, n_batches):
    for j in range(n_batches):
        winner, live, need, counts = t.live(j)
        assert need == 0 and live.shape[0] == 0 and rc.counts_dict(counts) == tc.ZERO_COUNTS
        assert not winner.view(np.uint32).any()   # (the wrapper's zeros: the call wrote nothing)
    assert tc.stats_dict(t.stats()) == tc.SPOILED_STATS


def test_capacity_and_spoiling(ramcrc, oracle_mod):
    full, more = _batches(oracle_mod, [[tc.capacity_lists(64)],
                                       [[tc.head(2), rc.obj(7, b"one more key", 1)]]])
    again = _batches(oracle_mod, [[tc.capacity_lists(64)[:9]]])[0]   # keys the table has
    t = ramcrc.ReplayTableHost(64, 8)
    tc.host_add(t, full)
    tc.host_add(t, again)
    tc.check_host(t, tc.expect(ramcrc, [full, again]), "exactly key_cap keys")
    assert t.stats()["keys"] == 64
    with pytest.raises(ramcrc.RamcrcError) as e:
        tc.host_add(t, more)
    assert e.value.code == ramcrc.EINVAL
    _spoiled(ramcrc, t, 3)
    with pytest.raises(ramcrc.RamcrcError):   # every add until the reset
        tc.host_add(t, again)
    _spoiled(ramcrc, t, 4)
    t.reset()
    tc.host_add(t, full)
    tc.check_host(t, tc.expect(ramcrc, [full]), "after the reset")
    t.close()
    t = ramcrc.ReplayTableHost(65, 8)
    for b in (full, again, more):
        tc.host_add(t, b)
    tc.check_host(t, tc.expect(ramcrc, [full, again, more]), "key_cap 65")
    assert t.stats()["keys"] == 65
    t.close()


def test_a_bad_segment_number_spoils(ramcrc, oracle_mod):
    b = _batches(oracle_mod, [[[tc.head(1)] + rc.tiny_entries()]])[0]
    t = ramcrc.ReplayTableHost(64, 4)
    tc.host_add(t, b)
    bad = tc.HostBatch.__new__(tc.HostBatch)
    bad.__dict__.update(b.__dict__)
    bad.table = b.table.copy()
    bad.table[2, 0] = 1   # = n_seg
    with pytest.raises(ramcrc.RamcrcError) as e:
        tc.host_add(t, bad)
    assert e.value.code == ramcrc.EINVAL
    _spoiled(ramcrc, t, 2)
    t.reset()
    tc.host_add(t, b)
    tc.check_host(t, tc.expect(ramcrc, [b]), "after the reset")


def test_max_batches(ramcrc, oracle_mod):
    b = _batches(oracle_mod, [[[tc.head(1)] + rc.tiny_entries()]])[0]
    t = ramcrc.ReplayTableHost(64, 2)
    tc.host_add(t, b)
    tc.host_add(t, b)
    with pytest.raises(ramcrc.RamcrcError) as e:
        tc.host_add(t, b)
    assert e.value.code == ramcrc.EINVAL
    tc.check_host(t, tc.expect(ramcrc, [b, b]), "still usable")
    for bad in (0, segments.REPLAY_TABLE_MAX_BATCHES + 1):
        with pytest.raises(ramcrc.RamcrcError):
            ramcrc.ReplayTableHost(64, bad)
    ramcrc.ReplayTableHost(64, segments.REPLAY_TABLE_MAX_BATCHES).close()


# --------------------------------------------------------- 7. list capacity
def test_list_capacity(ramcrc, relations):
    bs, exps = relations
    t, _ = _relations(ramcrc, relations)
    e_winner, e_live, e_counts = exps[2][1]
    need = e_live.shape[0]
    for cap in (need - 1, 0):
        winner, live, n, counts = t.live(1, live_cap=cap)
        assert n == need and np.array_equal(live, e_live[:cap]) and np.array_equal(winner, e_winner)
        assert rc.counts_dict(counts) == e_counts


# ----------------------------------------------------------------- 8. state
def test_state(ramcrc, relations, hot, oracle_mod):
    """One table: the relations, reset, the hot key, reset, the relations
    again; a second table fed alternately; an empty batch and one without
    participants."""
    bs, exps = relations
    t = ramcrc.ReplayTableHost(2000, 4)
    u = ramcrc.ReplayTableHost(2000, 4)
    for b in bs:
        tc.host_add(t, b)
        tc.host_add(u, hot)
    first = tc.check_host(t, exps[2], "relations")
    tc.check_host(u, tc.expect(ramcrc, [hot] * 3, python=False), "the other table")
    t.reset()
    tc.host_add(t, hot)
    tc.check_host(t, tc.expect(ramcrc, [hot], python=False), "hot")
    t.reset()
    for b in bs:
        tc.host_add(t, b)
    second = tc.check_host(t, exps[2], "relations again")
    for a, b in zip(first, second):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # a batch without participants, and one without records
    quiet = _batches(oracle_mod, [[[tc.head(3), pc.entry(pc.LOGDIGEST, b"d")]]])[0]
    empty = tc.HostBatch.__new__(tc.HostBatch)
    empty.__dict__.update(quiet.__dict__)
    empty.table = quiet.table[:0]
    t.reset()
    for b in (quiet, bs[0], empty):
        tc.host_add(t, b)
    got = tc.check_host(t, tc.expect(ramcrc, [quiet, bs[0], empty]), "quiet, relations 0, empty")
    assert (got[0][0]["batch"] == tc.NONE).all() and got[2][0].shape[0] == 0


# ---------------------------------------------------- 10. reference scenarios
def test_reference_scenarios(ramcrc, oracle_mod):
    ref = pc.load("replay_resolve_ref.json")
    lists, which = tc.reference_lists(ref)
    bs = _batches(oracle_mod, [[es] for es in lists])
    t = ramcrc.ReplayTableHost(256, len(bs))
    for b in bs:
        tc.host_add(t, b)
    exp = tc.expect(ramcrc, bs)
    tc.check_host(t, exp, "reference")
    tc.check_reference(ref, which, exp, bs)
