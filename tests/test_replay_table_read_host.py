"""ramcrc_replay_table_read_host: a multi-read's reply from the replay table on
the host, the loop of MasterService::multiRead (src/MasterService.cc:1352-1415)
over ObjectManager::readObject and rejectOperation (src/ObjectManager.cc:
324-369, :2893-2907).  The expectation is the plain Python of read_cases.py,
held against tests/golden/multi_read_ref.json and, through lookup_cases.py,
against the live query's winners before a call is held against it.  The device
tests (test_gpu_replay_table_read.py) run the same scenarios."""
import ctypes

import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import read_cases as rd
import replay_table_cases as tc
import resolve_cases as rc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return rd.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_and_helpers_match_the_abi():
    assert segments.REJECT_RULES_DTYPE.itemsize == 16 and segments.READ_SUMMARY_DTYPE.itemsize == 80
    assert segments.READ_PART_DTYPE.itemsize == 16
    assert segments.READ_SUMMARY_DTYPE.names == ("returned", "reply_bytes", "ok", "doesnt_exist",
                                                 "object_exists", "wrong_version", "bad", "value_bytes",
                                                 "key_bytes", "spoiled")
    r = segments.read_rules([None, dict(given_version=(1 << 63) + 5, exists=1), dict(version_ne_given=7)])
    assert r.tobytes() == bytes(16) + ((1 << 63) + 5).to_bytes(8, "little") + bytes([0, 1, 0, 0]) + \
        bytes(4) + bytes(8) + bytes([0, 0, 0, 7]) + bytes(4)
    reply = b"\0\0\0\0" + (9).to_bytes(8, "little") + b"\3\0\0\0abc" + b"\5\0\0\0" + bytes(8) + b"\7\0\0\0" + \
        b"\0" * 16
    assert segments.multi_read_parts(reply, 3) == [(0, 9, b"abc"), (5, 0, b""), (0, 0, b"")]
    assert segments.multi_read_parts(np.frombuffer(reply, np.uint8), 1) == [(0, 9, b"abc")]
    with pytest.raises(ValueError):
        segments.multi_read_parts(reply[:18], 1)


def test_the_expectation_matches_the_goldens():
    ref = rd.golden()
    assert rd.check_expectation_against_golden(ref) == 9
    assert [s["name"] for s in ref["scenarios"]] == ["multiRead_basics", "multiRead_noSuchObject",
                                                     "multiRead_bufferSizeExceeded"]


def test_goldens(drv):
    rd.case_goldens(drv)


def test_version_relations_across_batches(drv):
    rd.case_relations(drv)


def test_reject_rules(drv):
    rd.case_reject_rules(drv)


def test_multi_key_objects_in_both_modes(drv):
    rd.case_multi_key(drv)


def test_alignment(drv):
    rd.case_alignment(drv)


def test_copy_size_classes(drv):
    rd.case_size_classes(drv)


def test_truncation(drv):
    rd.case_truncation(drv)


def test_bad_queries_and_bad_rules_among_good_ones(drv):
    rd.case_bad_queries(drv)


def test_one_key_a_thousand_times(drv):
    rd.case_duplicates(drv)


def test_nullable_and_empty_arguments(drv):
    rd.case_nullable_and_empty(drv)


def test_read_only_and_reads_between_adds(drv, mixed):
    rd.case_read_only(drv, mixed)


def test_the_wrapper(ramcrc, drv):
    """ReplayTableHost.read: the same bytes through the Python wrapper."""
    b = drv.batch([[tc.head(1)] + rc.tiny_entries() + [rc.obj(1, b"w", 4, b"wrapped")]])
    tab = drv.table(64, 1)
    try:
        tab.add(b)
        ep = rd.checked(tab)
        keys = [(1, b"w"), (1, b"x"), (1, b"y"), (1, b"w")]
        kb, q = segments.lookup_queries(keys)
        rules = [None, None, dict(exists=1), None]
        for cap, value_only in ((rd.HUGE, False), (rd.HUGE, True), (40, True)):
            want = rd.Want(ep[0], ep[1], keys, rules, value_only, cap)
            reply, off, summary, results = tab.t.read(kb, q, cap, rules=segments.read_rules(rules),
                                                      value_only=value_only, want_results=True)
            assert reply.tobytes() == want.reply and off.tolist() == want.off
            assert rd.summary_dict(summary) == want.summary
            assert lc.same(results, tab.t.lookup(kb, q)[0])
            assert segments.multi_read_parts(reply, summary["returned"]) == want.parts
        assert tab.t.read(kb, q, rd.HUGE)[3] is None
    finally:
        tab.close()


def test_spoiled_tables(ramcrc, drv):
    """Spoiled by a bad segment number and by the key capacity: reply,
    part_off and results stay as they were, the summary says spoiled, and
    after the reset the table answers again."""
    b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
    bad = tc.HostBatch.__new__(tc.HostBatch)
    bad.__dict__.update(b.__dict__)
    bad.table = b.table.copy()
    bad.table[2, 0] = 1   # = n_seg
    full = drv.batch([tc.capacity_lists(64)])
    more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
    keys = [(1, b"x"), (7, b"cap key 3"), (1, b"absent"), (1, b"y")]
    kb, q = segments.lookup_queries(keys)
    for first, spoiler in ((b, bad), (full, more)):
        tab = drv.table(64, 4)
        try:
            tab.add(first)
            rd.read(tab, rd.checked(tab), keys, what="before")
            with pytest.raises(ramcrc.RamcrcError):
                tab.add(spoiler)
            g = tab.read_raw(kb, q, rd.HUGE)
            assert g.summary == rd.SPOILED_SUMMARY
            assert (g.reply_all == rd.FILL).all() and (g.off_all == rd.FILL64).all()
            assert (g.res_all == rd.FILL).all()
            tab.reset()
            tab.add(first)
            rd.read(tab, rd.checked(tab), keys, what="after the reset")
        finally:
            tab.close()


def test_bad_arguments(ramcrc):
    L = ramcrc.lib()
    t = ramcrc.ReplayTableHost(64, 1)
    q = np.zeros(1, segments.LOOKUP_KEY_DTYPE)
    s = np.zeros(1, segments.READ_SUMMARY_DTYPE)
    out = np.zeros(64, np.uint8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    call = lambda *a: L.ramcrc_replay_table_read_host(*a)
    E = ramcrc.EINVAL
    assert call(None, None, 0, vp(q), 1, None, None, 0, vp(out), 64, None, None, vp(s)) == E
    assert call(t._h, None, 0, None, 1, None, None, 0, vp(out), 64, None, None, vp(s)) == E
    assert call(t._h, None, 0, vp(q), 1, None, None, 0, vp(out), 64, None, None, None) == E
    assert call(t._h, None, 0, vp(q), 1, None, None, 2, vp(out), 64, None, None, vp(s)) == E
    assert call(t._h, None, 0, vp(q), 1, None, None, 0, None, 64, None, None, vp(s)) == E
    assert call(t._h, None, 8, vp(q), 1, None, None, 0, vp(out), 64, None, None, vp(s)) == E
    assert call(t._h, None, 0, vp(q), 0xFFFFFFFF, None, None, 0, vp(out), 64, None, None, vp(s)) == E
    assert not out.any() and not s.view(np.uint8).any()
    assert call(t._h, None, 0, vp(q), 1, None, None, 0, None, 0, None, None, vp(s)) == 0
    assert call(t._h, None, 0, None, 0, None, None, 0, None, 0, None, None, None) == 0
    t.close()
