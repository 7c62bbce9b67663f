"""ramcrc_replay_table_enumerate_host: one reply of a table enumeration from the
replay table on the host, MasterService::enumerate (src/MasterService.cc:409-456)
over Enumeration::complete (src/Enumeration.cc:269-351).  The expectation is
the plain Python of enumerate_cases.py, held against
tests/golden/enumerate_ref.json and, through lookup_cases.py, against the live
query's winners before a call is held against it.  The device tests
(test_gpu_replay_table_enumerate.py) run the same scenarios."""
import ctypes

import numpy as np
import pytest

from ramcloud_amd import segments

import enumerate_cases as en
import lookup_cases as lc
import replay_table_cases as tc
import resolve_cases as rc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return en.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_and_helpers_match_the_abi():
    assert segments.ENUM_FRAME_DTYPE.itemsize == 40 and segments.ENUMERATE_SUMMARY_DTYPE.itemsize == 88
    assert segments.ENUM_FRAME_DTYPE.names == ("tablet_start_hash", "tablet_end_hash", "num_buckets",
                                               "bucket_index", "bucket_next_hash")
    assert segments.ENUMERATE_SUMMARY_DTYPE.names == (
        "num_buckets", "next_bucket", "next_hash", "objects", "payload_bytes", "value_bytes", "key_bytes",
        "tombstones", "full", "stuck", "spoiled")
    payload = b"\3\0\0\0abc" + bytes(4) + b"\1\0\0\0z" + b"junk"
    assert segments.enumerate_objects(payload, 16) == [b"abc", b"", b"z"]
    assert segments.enumerate_objects(np.frombuffer(payload, np.uint8), 7) == [b"abc"]
    assert segments.enumerate_objects(payload, 0) == []
    for bad in (6, 9, 15, 21):
        with pytest.raises(ValueError):
            segments.enumerate_objects(payload, bad)
    f = segments.enum_frames([(0, 9, 4, 3, 7)])
    assert f.shape == (1,) and tuple(int(x) for x in f[0]) == (0, 9, 4, 3, 7)
    assert segments.enum_frames([]).shape == (0,)
    for bad in ([(0, 9, 0, 0, 0)], [(0, 9, 6, 0, 0)], [(0, 1, 1, 0, 0)] * 9):
        with pytest.raises(ValueError):
            segments.enum_frames(bad)


def test_the_expectation_matches_the_goldens(drv):
    ref = en.golden()
    assert en.check_expectation_against_golden(ref, drv) == 3
    assert [s["name"] for s in ref["scenarios"]] == [
        "MasterServiceTest.enumerate_basics", "MasterServiceTest.enumerate_mergeTablet",
        "TableEnumeratorTest.keysOnly"]


def test_the_cases_straddle_the_kernels_thresholds():
    """The tile, scan-step and size-class thresholds the cases are built around
    are the kernel sources' own: if one moves, this fails instead of the cases
    going blind."""
    assert en.source_constants() == dict(kPartThreads=en.TILE, kAppBigMin=en.BIG_MIN, kAppGroupMin=en.GROUP_MIN,
                                         kEnScanPer=en.SCAN_PER)


def test_goldens(drv):
    en.case_goldens(drv)


def test_buckets_of_one_to_forty_keys_and_every_cut(drv):
    en.case_buckets(drv)


def test_wrap_and_tile_edges(drv):
    en.case_wrap_and_tile_edges(drv)


def test_bucket_limit_at_every_value(drv):
    en.case_every_limit(drv)


def test_selection(drv):
    en.case_selection(drv)


def test_more_tiles_than_a_step_of_the_scan(drv):
    en.case_many_tiles(drv)


def test_alignment_and_size_classes(drv):
    en.case_size_classes(drv)


def test_multi_key_objects_and_broken_key_tables(drv):
    en.case_multi_key(drv)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_cursor_walk_gives_every_object_once(drv, seed):
    en.case_random_walks(drv, seed)


def test_read_only(drv, mixed):
    en.case_read_only(drv, mixed)


def test_stuck(drv):
    """The first object alone does not fit: full and stuck, nothing sent, the
    cursor where it was; with room for it the walk goes on."""
    tab, hash_of = en.placed_table(drv, 32, [(5, 1, 2, 30), (6, 1, 1, 2)])
    try:
        ep = en.checked(tab)
        one = en.Want(ep[0], ep[1], hash_of, tab.S, en.Args(1)).ends[0]
        for bucket, mb in ((5, 0), (5, 3), (5, one - 1)):
            g, w = en.ask(tab, ep, hash_of, en.Args(1, bucket=bucket, max_bytes=mb), what=("stuck", mb))
            assert (g.summary["stuck"], g.summary["full"], g.summary["objects"]) == (1, 1, 0)
            assert (g.summary["next_bucket"], g.summary["next_hash"]) == (5, 5) and g.payload == b""
        # two keys of one hash: the cut moves back before both, which leaves nothing
        g, w = en.ask(tab, ep, hash_of, en.Args(1, bucket=5, max_bytes=one), what="one of two of a hash fits")
        assert g.summary["stuck"] == 1 and g.summary["payload_bytes"] == 0
        # from an earlier bucket the cursor moves to bucket 5 first: not stuck
        g, w = en.ask(tab, ep, hash_of, en.Args(1, bucket=2, max_bytes=3), what="a later bucket is left out")
        assert (g.summary["stuck"], g.summary["full"], g.summary["next_bucket"]) == (0, 1, 5)
        g, w = en.ask(tab, ep, hash_of, en.Args(1, bucket=5, max_bytes=2 * one + 1), what="room for the hash")
        assert (g.summary["stuck"], g.summary["objects"], g.summary["next_bucket"]) == (0, 2, 6)
    finally:
        tab.close()


def test_the_wrapper(ramcrc, drv):
    """ReplayTableHost.enumerate: the same bytes through the Python wrapper."""
    tab, hash_of = en.placed_table(drv, 32, [(5, 1, 3, 30), (6, 1, 1, 2), (9, 2, 1, 2)])
    try:
        ep = en.checked(tab)
        for a in (en.Args(1), en.Args(1, max_bytes=100), en.Args(1, keys_only=True, bucket=5, next_hash=5, limit=6),
                  en.Args(1, stale=[(0, en.MAXH, 16, 6, 0)]), en.Args(2, capacity=0)):
            want = en.Want(ep[0], ep[1], hash_of, tab.S, a)
            payload, summary = tab.t.enumerate(
                a.table_id, a.max_bytes, first_hash=a.first, last_hash=a.last, bucket_index=a.bucket,
                bucket_next_hash=a.next_hash, bucket_limit=a.limit, stale=a.stale, keys_only=a.keys_only,
                payload_capacity=a.capacity)
            assert payload.tobytes() == want.payload and en.summary_dict(summary) == want.summary
            assert segments.enumerate_objects(payload, summary["payload_bytes"]) == want.entries
    finally:
        tab.close()


def test_spoiled_tables(ramcrc, drv):
    """Spoiled by the key capacity: the payload stays as it was, the summary
    says spoiled, and after the reset the table answers again."""
    full = drv.batch([tc.capacity_lists(64)])
    more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
    tab = en.table(drv, 64, 4)
    try:
        tab.add(full)
        g, _ = en.ask(tab, en.checked(tab), en.key_hash, en.Args(7), what="before")
        assert g.summary["objects"] == 64
        with pytest.raises(ramcrc.RamcrcError):
            tab.add(more)
        g = en.host_call(ramcrc, tab.t, en.Args(7), 256, 256)
        assert g.summary == en.SPOILED_SUMMARY and (g.payload_all == en.FILL).all()
        tab.reset()
        tab.add(full)
        en.ask(tab, en.checked(tab), en.key_hash, en.Args(7), what="after the reset")
    finally:
        tab.close()


def test_bad_arguments(ramcrc):
    t = ramcrc.ReplayTableHost(64, 1)   # S = 128
    S = 128
    E = ramcrc.EINVAL
    ok = en.Args(1)
    code = lambda a, **kw: en.host_raw(ramcrc, t, a, 64, kw.pop("capacity", 64), **kw)
    assert code(ok)[0] == 0 and code(ok)[1].summary == dict(en.ZERO_SUMMARY, num_buckets=S, next_bucket=S)
    for flags in (2, 3, 1 << 31):
        assert code(ok, flags=flags)[0] == E                                   # unknown flag bits
    assert code(ok.but(bucket=S))[0] == 0 and code(ok.but(bucket=S + 1))[0] == E
    assert code(ok.but(bucket=5, limit=4))[0] == E and code(ok.but(bucket=5, limit=5))[0] == 0
    assert code(ok.but(limit=S))[0] == 0 and code(ok.but(limit=S + 1))[0] == E
    for nb in (0, 3, 6, (1 << 63) + 1):
        bad = np.zeros(2, segments.ENUM_FRAME_DTYPE)
        bad["num_buckets"] = (4, nb)
        c, g = code(ok, stale_raw=bad)
        assert c == E and (g.summary_raw == en.FILL).all()
    L = ramcrc.lib().ramcrc_replay_table_enumerate_host
    s = np.zeros(1, segments.ENUMERATE_SUMMARY_DTYPE)
    out = np.zeros(64, np.uint8)
    fr = np.zeros(9, segments.ENUM_FRAME_DTYPE)
    fr["num_buckets"] = 1
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L(None, 1, 0, 0, 0, 0, 0, None, 0, 0, vp(out), 64, 64, vp(s)) == E
    assert L(t._h, 1, 0, 0, 0, 0, 0, None, 0, 0, vp(out), 64, 64, None) == E        # no summary
    assert L(t._h, 1, 0, 0, 0, 0, 0, None, 0, 0, None, 64, 64, vp(s)) == E          # no payload
    assert L(t._h, 1, 0, 0, 0, 0, 0, None, 1, 0, vp(out), 64, 64, vp(s)) == E       # no frames
    assert L(t._h, 1, 0, 0, 0, 0, 0, vp(fr), 9, 0, vp(out), 64, 64, vp(s)) == E     # too many frames
    assert not out.any() and not s.view(np.uint8).any()
    assert L(t._h, 1, 0, 0, 0, 0, 0, vp(fr), 8, 0, vp(out), 64, 64, vp(s)) == 0
    assert L(t._h, 1, 0, 0, 0, 0, 0, None, 0, 0, None, 0, 64, vp(s)) == 0
    t.close()
