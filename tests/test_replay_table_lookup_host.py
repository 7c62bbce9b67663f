"""ramcrc_replay_table_lookup_host: what the replay table holds for a key, the
batched form of ObjectManager::lookup / readObject (src/ObjectManager.cc:
2704-2741, :325-369) against the table of ramcrc_replay_table_*_host.  The
expectation is the plain-Python replay of lookup_cases.py, held against the
live query's winners for every participant before the lookup is held against
it.  The device tests (test_gpu_replay_table_lookup.py) run the same scenarios."""
import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import replay_table_cases as tc
import resolve_cases as rc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return lc.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_match_the_abi():
    assert segments.LOOKUP_KEY_DTYPE.itemsize == 24 and segments.LOOKUP_RESULT_DTYPE.itemsize == 32
    assert segments.LOOKUP_COUNTS_DTYPE.itemsize == 40
    assert segments.LOOKUP_COUNTS_DTYPE.names == ("objects", "tombstones", "absent", "bad", "spoiled")
    kb, q = segments.lookup_queries([(1, b"ab"), (2, b""), (3, b"cde")], align=4)
    assert kb.tobytes() == b"ab\0\0cde" and q["key_off"].tolist() == [0, 4, 4]
    assert q["key_len"].tolist() == [2, 0, 3] and q["table_id"].tolist() == [1, 2, 3]


def test_empty_and_fresh_tables(drv):
    lc.case_empty_and_fresh(drv)


def test_version_relations_across_batches(drv):
    lc.case_relations(drv)


def test_key_identity(drv):
    lc.case_identity(drv)


def test_the_longest_key(drv):
    lc.case_longest_key(drv)


def test_one_probe_chain(drv):
    lc.case_one_chain(drv)


def test_collisions_of_the_seed(drv):
    lc.case_seed_collisions(drv)


def test_given_and_computed_hashes_mix(drv, mixed):
    lc.case_mixed_hashes(drv, mixed)


def test_an_absent_key_on_a_claimed_slot(drv):
    lc.case_absent_on_a_claimed_slot(drv)


def test_multi_key_objects(drv):
    lc.case_multi_key(drv)


def test_bad_queries_among_good_ones(drv):
    lc.case_bad_queries(drv)


def test_duplicates(drv):
    lc.case_duplicates(drv)


def test_exhaustive_cross_check(drv, mixed):
    lc.case_exhaustive(drv, mixed)


def test_read_only(drv, mixed):
    lc.case_read_only(drv, mixed)


def test_nullable_and_empty_arguments(drv):
    lc.case_nullable_and_empty(drv)


def test_reference_scenarios(drv):
    lc.case_reference(drv)


def test_spoiled_tables(ramcrc, drv):
    """Spoiled by a bad segment number and by the key capacity: the results
    stay as they were, the counts say spoiled, and after the reset the table
    answers again."""
    b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
    bad = tc.HostBatch.__new__(tc.HostBatch)
    bad.__dict__.update(b.__dict__)
    bad.table = b.table.copy()
    bad.table[2, 0] = 1   # = n_seg
    full = drv.batch([tc.capacity_lists(64)])
    more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
    keys = [(1, b"x"), (7, b"cap key 3"), (1, b"absent")]
    kb, q = segments.lookup_queries(keys)
    for first, spoiler in ((b, bad), (full, more)):
        tab = drv.table(64, 4)
        try:
            tab.add(first)
            lc.lookup(tab, lc.checked_expectation(tab), keys, what="before")
            with pytest.raises(ramcrc.RamcrcError):
                tab.add(spoiler)
            res, counts = tab.t.lookup(kb, q)
            assert lc.counts_dict(counts) == lc.SPOILED_COUNTS
            assert not res.view(np.uint8).any()   # (the wrapper's zeros: the call wrote nothing)
            tab.reset()
            tab.add(first)
            lc.lookup(tab, lc.checked_expectation(tab), keys, what="after the reset")
        finally:
            tab.close()


def test_bad_arguments(ramcrc):
    import ctypes
    L = ramcrc.lib()
    t = ramcrc.ReplayTableHost(64, 1)
    q = np.zeros(1, segments.LOOKUP_KEY_DTYPE)
    r = np.zeros(1, segments.LOOKUP_RESULT_DTYPE)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.ramcrc_replay_table_lookup_host(None, None, 0, vp(q), 1, None, vp(r), None) == ramcrc.EINVAL
    assert L.ramcrc_replay_table_lookup_host(t._h, None, 0, None, 1, None, vp(r), None) == ramcrc.EINVAL
    assert L.ramcrc_replay_table_lookup_host(t._h, None, 0, vp(q), 1, None, None, None) == ramcrc.EINVAL
    assert L.ramcrc_replay_table_lookup_host(t._h, None, 8, vp(q), 1, None, vp(r), None) == ramcrc.EINVAL
    assert L.ramcrc_replay_table_lookup_host(t._h, None, 0, vp(q), 0xFFFFFFFF, None, vp(r), None) == ramcrc.EINVAL
    assert L.ramcrc_replay_table_lookup_host(t._h, None, 0, None, 0, None, None, None) == 0
    t.close()
