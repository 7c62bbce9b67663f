"""ramcrc_replay_table_index_build_host and ramcrc_index_lookup_host: the
secondary index over the replay table and IndexletManager::lookupIndexKeys
(src/IndexletManager.cc:611-709) on the host.  The expectation is the plain
Python of index_cases.py, held against tests/golden/index_ref.json and, through
lookup_cases.py, against the live query's winners before a call is held
against it.  The device tests (test_gpu_replay_index.py) run the same
scenarios."""
import numpy as np
import pytest

from ramcloud_amd import segments

import index_cases as ix
import lookup_cases as lc

T = ix.source_constants()["kIxTile"]


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return ix.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_and_helpers_match_the_abi():
    assert segments.INDEX_ENTRY_DTYPE.itemsize == 32 and segments.INDEX_BUILD_SUMMARY_DTYPE.itemsize == 56
    assert segments.INDEX_QUERY_DTYPE.itemsize == 40 and segments.INDEX_RESULT_DTYPE.itemsize == 48
    assert segments.INDEX_LOOKUP_SUMMARY_DTYPE.itemsize == 48
    assert segments.INDEX_BUILD_SUMMARY_DTYPE.names == (
        "n_entries", "key_bytes", "entries_needed", "key_bytes_needed", "objects_seen", "overflow", "spoiled")
    assert segments.INDEX_LOOKUP_SUMMARY_DTYPE.names == (
        "served", "hashes", "bad", "maxed_out", "n_entries", "overflow_index")
    kb, q = segments.index_queries([(b"ab", b"c", 7, 9), (b"", b"", 0, 1)], align=4)
    assert kb.tobytes() == b"ab\0\0c\0\0\0" and q.shape == (2,)
    assert tuple(int(x) for x in q[0]) == (0, 4, 7, 2, 1, 9, 0) and tuple(int(x) for x in q[1]) == (8, 8, 0, 0, 0, 1, 0)
    res = np.zeros(3, segments.INDEX_RESULT_DTYPE)
    res[0] = (0, 0, 0, 0, 2, 0, segments.INDEX_OK, 0)
    res[1] = (segments.READ_NONE, 0, 0, 0, 0, 0, segments.INDEX_BAD_QUERY, 0)
    res[2] = (2, 5, 99, 1, 1, 2, segments.INDEX_OK, 0)
    reply = segments.index_lookup_hashes(np.array([11, 12, 13], np.uint64), res, np.frombuffer(b"xyz", np.uint8))
    assert [(s, h.tolist(), k, n) for s, h, k, n in reply] == [
        (0, [11, 12], None, 0), (1, [], None, 0), (0, [13], b"yz", 99)]
    assert segments.index_lookup_hashes(np.array([11, 12, 13], np.uint64), res)[2][2] == (1, 2)
    with pytest.raises(ValueError):
        segments.index_lookup_hashes(np.array([11, 12], np.uint64), res)


def test_the_expectation_matches_the_goldens():
    ref = ix.golden()
    assert ix.check_expectation_against_golden(ref) == 8
    assert len(ref["key_compare"]) == 10


def test_goldens(drv):
    ix.case_goldens(drv)


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T, 5 * T + 3])
def test_sort_edges_ascending_descending_equal(drv, n):
    ix.case_sort(drv, n)


def test_sort_with_room_to_spare(drv):
    ix.case_sort(drv, T + 1, extra=2 * T)


def test_comparator(drv):
    ix.case_comparator(drv)


def test_selection(drv):
    ix.case_selection(drv)


def test_capacity(drv):
    ix.case_capacity(drv)


def test_lookup(drv):
    ix.case_lookup(drv)


def test_long_runs(drv):
    ix.case_long_runs(drv)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_chain_build_lookup_read_hashes(drv, seed):
    ix.case_chain(drv, seed)


def test_read_only(drv, mixed):
    ix.case_read_only(drv, mixed)


def test_the_wrappers(drv):
    """ReplayTableHost.index_build sizes by itself; index_lookup_host and
    segments.index_lookup_hashes give the reply."""
    objs = ix.lookup_table(drv)
    tab = ix.hashed_table(drv, 64, objs)
    try:
        idx = tab.t.index_build(1, 1)
        pairs = sorted((k, h) for _, k, h in objs)
        assert int(idx.summary["n_entries"]) == len(pairs) == idx.entries.shape[0] == idx.hashes.shape[0]
        assert ix.normalized(idx.entries, idx.index_keys) == ix.WantIndex(pairs, len(pairs)).entries
        ranges = [(b"run", b"run", 15, 2), (b"", b"", 0, 3)]
        kb, q = segments.index_queries(ranges)
        out, results, sm = drv.ramcrc.index_lookup_host(idx, kb, q)
        want, wsm = ix.expect_lookup(pairs, ranges)
        got = [(s, h.tolist(), k, n) for s, h, k, n in segments.index_lookup_hashes(out, results, idx.index_keys)]
        assert got == want and ix.sdict(sm, ix.LSUM.names) == wsm
        small = tab.t.index_build(1, 1, entry_capacity=3)
        assert int(small.summary["overflow"]) == 1 and small.entries.shape[0] == 0
    finally:
        tab.close()


def test_spoiled_and_bad_arguments(drv, ramcrc):
    """A spoiled table: outputs untouched, summary zero with spoiled = 1, and a
    lookup against that build serves nothing.  index_id 0, NULL arrays with a
    capacity and a NULL summary are EINVAL with nothing written."""
    import replay_table_cases as tc
    import resolve_cases as rc
    tab = drv.table(64, 4)
    try:
        tab.add(drv.batch([tc.capacity_lists(64)]))
        with pytest.raises(ramcrc.RamcrcError):
            tab.add(drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]]))
        g = ix.host_build(ramcrc, tab.t, 7, 1, 8, 64)
        assert g.summary == dict(ix.ZERO_BSUM, spoiled=1) and g.entries == []
        ix.lookup(drv, g, [], [(b"", b"", 0, 4)], what="a spoiled build", dead=True)
        tab.reset()
        for iid, ecap, kcap, null in ((0, 8, 64, False), (1, 8, 64, True), (1, 0, 64, True)):
            code, g = ix.host_build_raw(ramcrc, tab.t, 7, iid, ecap, kcap, null)
            assert code == ramcrc.EINVAL, (iid, ecap, kcap, null)
            assert (g.entries_all == ix.FILL).all() and (g.keys_all == ix.FILL).all()
            assert g.summary == dict.fromkeys(ix.BSUM.names, 0xA5A5A5A5A5A5A5A5)
        z = np.zeros(64, np.uint64)
        L = ramcrc.lib().ramcrc_replay_table_index_build_host
        assert L(tab.t._h, 7, 1, z.ctypes.data, 1 << 32, z.ctypes.data, z.ctypes.data, 8, z.ctypes.data) == ramcrc.EINVAL
        assert L(tab.t._h, 7, 1, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data, 8, None) == ramcrc.EINVAL
        assert L(None, 7, 1, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data, 8, z.ctypes.data) == ramcrc.EINVAL
        assert not z.any()
    finally:
        tab.close()
