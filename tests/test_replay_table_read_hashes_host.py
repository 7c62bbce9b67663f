"""ramcrc_replay_table_read_hashes_host: an indexed read's reply from the replay
table on the host, the loop of MasterService::readHashes
(src/MasterService.cc:797-809) over ObjectManager::readHashes
(src/ObjectManager.cc:179-265).  The expectation is the plain Python of
read_hashes_cases.py, held against tests/golden/read_hashes_ref.json and,
through lookup_cases.py, against the live query's winners before a call is held
against it.  The device tests (test_gpu_replay_table_read_hashes.py) run the
same scenarios."""
import ctypes

import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import read_hashes_cases as rh
import replay_table_cases as tc
import resolve_cases as rc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return rh.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_and_helpers_match_the_abi():
    assert segments.HASH_PART_DTYPE.itemsize == 16 and segments.READ_HASHES_SUMMARY_DTYPE.itemsize == 72
    assert segments.HASH_PART_DTYPE.names == ("off", "objects", "reserved")
    assert segments.READ_HASHES_SUMMARY_DTYPE.names == (
        "hashes", "objects", "objects_counted", "reply_bytes", "value_bytes", "key_bytes", "empty",
        "tombstones", "spoiled")
    reply = (9).to_bytes(8, "little") + b"\3\0\0\0abc" + bytes(8) + bytes(4) + (1 << 63).to_bytes(8, "little") + \
        b"\1\0\0\0z"
    assert segments.read_hashes_objects(reply, 3) == [(9, b"abc"), (0, b""), (1 << 63, b"z")]
    assert segments.read_hashes_objects(np.frombuffer(reply, np.uint8), 1) == [(9, b"abc")]
    with pytest.raises(ValueError):
        segments.read_hashes_objects(reply[:14], 1)
    with pytest.raises(ValueError):
        segments.read_hashes_objects(reply[:10], 1)


def test_the_expectation_matches_the_goldens():
    ref = rh.golden()
    assert rh.check_expectation_against_golden(ref) == 3
    assert [s["name"] for s in ref["scenarios"]] == ["ObjectManagerTest.readHashes",
                                                     "MasterServiceTest.readHashes", "RamCloudTest.readHashes"]


def test_the_cases_straddle_the_kernels_thresholds():
    """The tile and size-class thresholds the cases are built around are the
    kernel sources' own: if one moves, this fails instead of the cases going
    blind."""
    assert rh.source_constants() == dict(kPartThreads=rh.TILE, kAppBigMin=rh.BIG_MIN, kAppGroupMin=rh.GROUP_MIN)


def test_goldens(drv):
    rh.case_goldens(drv)


def test_version_relations_across_batches(drv):
    rh.case_relations(drv)


def test_fan_out_under_one_caller_hash(drv):
    rh.case_fan_out(drv)


def test_seed_collisions(drv):
    rh.case_seed_collisions(drv)


def test_mixed_hashes(drv, mixed):
    rh.case_mixed_hashes(drv, mixed)


def test_after_a_clean(drv, mixed):
    rh.case_after_a_clean(drv, mixed)


def test_multi_key_objects_and_broken_key_tables(drv):
    rh.case_multi_key(drv)


def test_alignment_and_size_classes(drv):
    rh.case_alignment_and_size_classes(drv)


def test_truncation(drv):
    rh.case_truncation(drv)


def test_cuts_at_tile_edges(drv):
    rh.case_tile_edges(drv)


def test_one_hash_a_thousand_times(drv):
    rh.case_repeats(drv)


def test_nullable_and_empty_arguments(drv):
    rh.case_nullable_and_empty(drv)


def test_read_only_and_calls_between_adds(drv, mixed):
    rh.case_read_only(drv, mixed)


def test_the_wrapper(ramcrc, drv):
    """ReplayTableHost.read_hashes: the same bytes through the Python wrapper."""
    tab, hash_of = rh.truncation_table(drv)
    try:
        ep = rh.checked(tab)
        asked = [60, 101, 50, 999, 107, 60]
        for ml, cap in ((rh.HUGE, None), (40, None), (rh.HUGE, 60), (0, 0)):
            want = rh.Want(ep[0], ep[1], hash_of, 1, asked, ml, cap)
            reply, parts, summary = tab.t.read_hashes(1, asked, ml, reply_capacity=cap)
            assert reply.tobytes() == want.reply and rh.summary_dict(summary) == want.summary
            assert [tuple(int(x) for x in p) for p in parts] == want.parts
            assert segments.read_hashes_objects(reply, summary["objects"]) == want.objects
    finally:
        tab.close()


def test_spoiled_tables(ramcrc, drv):
    """Spoiled by a bad segment number and by the key capacity: reply and parts
    stay as they were, the summary says spoiled, and after the reset the table
    answers again."""
    b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
    bad = tc.HostBatch.__new__(tc.HostBatch)
    bad.__dict__.update(b.__dict__)
    bad.table = b.table.copy()
    bad.table[2, 0] = 1   # = n_seg
    full = drv.batch([tc.capacity_lists(64)])
    more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
    for first, spoiler, tid, key in ((b, bad, 1, b"y"), (full, more, 7, b"cap key 3")):
        asked = [rh.key_hash((tid, key)), 5]
        tab = drv.table(64, 4)
        try:
            tab.add(first)
            g, _ = rh.ask(tab, rh.checked(tab), rh.key_hash, tid, asked, what="before")
            assert g.summary["objects"] == 1
            with pytest.raises(ramcrc.RamcrcError):
                tab.add(spoiler)
            g = rh.host_call(ramcrc, tab.t, tid, asked, 256, 256, rh.HUGE)
            assert g.summary == rh.SPOILED_SUMMARY
            assert (g.reply_all == rh.FILL).all() and (g.parts_all == rh.FILL).all()
            tab.reset()
            tab.add(first)
            rh.ask(tab, rh.checked(tab), rh.key_hash, tid, asked, what="after the reset")
        finally:
            tab.close()


def test_bad_arguments(ramcrc):
    L = ramcrc.lib()
    t = ramcrc.ReplayTableHost(64, 1)
    h = np.zeros(1, np.uint64)
    s = np.zeros(1, segments.READ_HASHES_SUMMARY_DTYPE)
    out = np.zeros(64, np.uint8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    call = lambda *a: L.ramcrc_replay_table_read_hashes_host(*a)
    E = ramcrc.EINVAL
    assert call(None, 1, vp(h), 1, 0, vp(out), 64, 64, None, vp(s)) == E
    assert call(t._h, 1, vp(h), 1, 1, vp(out), 64, 64, None, vp(s)) == E            # flags
    assert call(t._h, 1, vp(h), 1, 1 << 31, vp(out), 64, 64, None, vp(s)) == E
    assert call(t._h, 1, vp(h), 1, 0, vp(out), 64, 64, None, None) == E             # no summary
    assert call(t._h, 1, None, 0, 0, None, 0, 0, None, None) == E                    # not even for no hashes
    assert call(t._h, 1, None, 1, 0, vp(out), 64, 64, None, vp(s)) == E             # no hashes
    assert call(t._h, 1, vp(h), 1, 0, None, 64, 64, None, vp(s)) == E               # no reply
    assert call(t._h, 1, vp(h), 0xFFFFFFFF, 0, vp(out), 64, 64, None, vp(s)) == E
    assert not out.any() and not s.view(np.uint8).any()
    assert call(t._h, 1, vp(h), 1, 0, None, 0, 0, None, vp(s)) == 0
    assert call(t._h, 1, None, 0, 0, None, 0, 0, None, vp(s)) == 0
    t.close()
