"""ramcrc_replay_table_clean_host and ramcrc_replay_table_clean_size_host:
cleaning batches out of the replay table on the host, the relocation step of
the log cleaner (LogCleaner::relocateLiveEntries, src/LogCleaner.cc:575-722,
over ObjectManager::relocateObject and relocateTombstone).  The expectation is
the plain Python of clean_cases.py, pinned by the properties listed there
against lookup, read, live, the oracle's walk and the oracle's certificate.
The device tests (test_gpu_replay_table_clean.py) run the same scenarios."""
import ctypes

import numpy as np
import pytest

from ramcloud_amd import segments

import clean_cases as cc
import lookup_cases as lc


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod):
    return cc.HostDriver(ramcrc, oracle_mod)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_dtypes_match_the_abi():
    assert segments.CLEAN_USAGE_DTYPE.itemsize == 32 and segments.CLEAN_SUMMARY_DTYPE.itemsize == 112
    assert segments.CLEAN_USAGE_DTYPE.names == ("records", "live_objects", "live_tombstones", "live_bytes")
    assert segments.CLEAN_SUMMARY_DTYPE.names == (
        "victims", "records", "moved_objects", "moved_tombstones", "object_bytes", "tombstone_bytes",
        "dropped_objects", "dropped_tombstones", "dropped_other", "needed_bytes", "needed_records", "out_bytes",
        "batch", "spoiled")


def test_slot_relations(drv):
    cc.case_relations(drv)


def test_tile_edges(drv):
    cc.case_tile_edges(drv)


def test_entry_shapes(drv):
    cc.case_entry_shapes(drv)


def test_non_participants(drv):
    cc.case_non_participants(drv)


def test_space(drv):
    cc.case_space(drv)


def test_handle_state(drv):
    cc.case_handle_state(drv)


def test_many_victims(drv):
    cc.case_many_victims(drv)


def test_closing_the_loop(drv, mixed):
    cc.case_closing_the_loop(drv, mixed)


def test_bad_arguments(ramcrc):
    """Rule 10 on the host: missing outputs, a capacity that is no multiple of
    16 and a record capacity of 2^32 are RAMCRC_EINVAL, and nothing changes."""
    t = ramcrc.ReplayTableHost(64, 4)
    try:
        seg = np.zeros(64, np.uint8)
        t.add(seg, 64, 1, np.array([[1, 0, 0, 0]], np.uint32), np.zeros((0, 4), np.uint32))
        z = np.full(1024, cc.FILL, np.uint8)
        at = lambda o: ctypes.c_void_p(z.ctypes.data + o)
        vic = np.array([0], np.uint32)
        good = dict(t=t._h, vic=ctypes.c_void_p(vic.ctypes.data), n=1, out=at(0), cap=64, cert=at(64),
                    status=at(80), entries=at(96), ecap=4, n_entries=at(160), work=at(176), summary=at(256))
        cases = [dict(t=None), dict(vic=None), dict(n=0), dict(summary=None), dict(cert=None), dict(status=None),
                 dict(n_entries=None), dict(entries=None), dict(work=None), dict(out=None), dict(cap=72),
                 dict(ecap=1 << 32)]
        L = ramcrc.lib()
        for change in cases:
            a = dict(good, **change)
            rc = L.ramcrc_replay_table_clean_host(a["t"], a["vic"], a["n"], a["out"], a["cap"], a["cert"],
                                                  a["status"], a["entries"], a["ecap"], a["n_entries"], a["work"],
                                                  None, None, a["summary"], None)
            assert rc == ramcrc.EINVAL, change
        for a in (dict(t=None), dict(vic=None), dict(n=0), dict(summary=None)):
            a = dict(good, **a)
            assert L.ramcrc_replay_table_clean_size_host(a["t"], a["vic"], a["n"], None, a["summary"]) == ramcrc.EINVAL
        assert (z == cc.FILL).all() and int(t.stats()["batches"]) == 1
        t.live(0)
    finally:
        t.close()


def test_the_wrappers_after_a_clean(drv, ramcrc):
    """Rule 5 through ReplayTableHost itself, which keeps a list of its batches'
    arrays: after a clean whose record table is longer than the survivors (the
    rows past the count hold the fill), lookup, read, write, remove, live and
    stats take the survivor as any batch and pass over the cleaned one."""
    import replay_table_cases as tc
    import resolve_cases as rc
    b0 = drv.batch([[tc.head(1)] + [rc.obj(1, b"k%d" % i, 1, b"value %d" % i * (i + 1)) for i in range(6)]],
                   cap=4096)
    b1 = drv.batch([[rc.obj(1, b"k0", 2, b"newer"), rc.tomb(1, b"k1", 1)]], cap=4096)
    t = ramcrc.ReplayTableHost(64, 8)
    try:
        for b in (b0, b1):
            tc.host_add(t, b)
        keys = [(1, b"k%d" % i) for i in range(6)] + [(1, b"nobody")]
        kb, q = segments.lookup_queries(keys)
        res0, _ = t.lookup(kb, q)
        reply0, off0, sm0, _ = t.read(kb, q, 1 << 20)
        o = t.clean([0], 4096, 64, fill=cc.FILL)
        n = int(o["n_entries"][0])
        assert o["batch"] == 2 and n == 4 and (o["entries"][n:] == cc.FILL32).all()
        res1, counts1 = t.lookup(kb, q)
        assert (res1["kind"] == res0["kind"]).all() and (res1["version"] == res0["version"]).all()
        assert res1["batch"].tolist() == [1, 1, 2, 2, 2, 2, segments.RESOLVE_NONE]
        reply1, off1, sm1, _ = t.read(kb, q, 1 << 20)
        assert reply1.tobytes() == reply0.tobytes() and cc.lc.same(off1, off0) and sm1 == sm0
        with pytest.raises(ramcrc.RamcrcError) as e:
            t.live(0)
        assert e.value.code == ramcrc.EINVAL
        winner, live, need, _ = t.live(2)
        assert need == n and winner.shape[0] == n and live[:, 0].tolist() == list(range(n))
        assert int(t.stats()["batches"]) == 3 and int(t.stats()["keys"]) == 6
        # a write over a moved key and a remove of another: old plus one, and the moved version
        data, reqs = segments.write_requests([(1, b"k2", b"written after the clean")])
        out, cert, parts, refs, old, wsm = t.write(data, reqs, 4096, 1, batch_segment_id=[10, 11, 12], want_old=True)
        assert int(wsm["ok"]) == 1 and int(parts["version"][0]) == 2 and int(old["batch"][0]) == 2
        out, cert, parts, refs, old, rsm = t.remove(kb, q[3:4], 4096, 1, batch_segment_id=[10, 11, 12], want_old=True)
        assert int(rsm["removed"]) == 1 and int(parts["version"][0]) == 1 and int(old["batch"][0]) == 2
        # and a clean of the survivor itself, through the kept arrays
        o2 = t.clean([2, 1], 4096, 64, fill=cc.FILL)
        assert o2["batch"] == 3 and int(o2["n_entries"][0]) == 6
        reply2, _, _, _ = t.read(kb, q, 1 << 20)
        assert reply2.tobytes() == reply0.tobytes()
    finally:
        t.close()
