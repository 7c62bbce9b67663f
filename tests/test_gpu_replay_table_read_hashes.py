"""ramcrc_replay_table_read_hashes_device: an indexed read's reply packed on the
GPU (k_rh_size, k_rh_scan, k_rh_gather), the loop of MasterService::readHashes
(src/MasterService.cc:797-809) over ObjectManager::readHashes
(src/ObjectManager.cc:179-265).

The scenarios are read_hashes_cases.py's, the ones
test_replay_table_read_hashes_host.py runs on the host: every batch is walked
by ctx.segment_walk, the expectation (plain Python, held against the goldens
and the live query's winners) is what every device call is held against, and a
host table fed the same batches must give the same bytes.  Reply, parts and
summary are pre-filled with 0xA5 and checked past their ends."""
import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import partition_cases as pc
import read_hashes_cases as rh
import replay_table_cases as tc
import resolve_cases as rc
from test_gpu_replay_table_lookup import grid_case  # noqa: F401  (the 249,165-record table)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = rh.FILL


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return rh.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_goldens(drv):
    assert rh.check_expectation_against_golden(rh.golden()) == 3
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


# --------------------------------------------------------------- grid size
def test_small_grids(ramcrc, grid_case):  # noqa: F811
    """250,000 hashes, every second one the Key::getHash of a key of batch 0 in
    a shuffled order, the others of keys nobody has, against the 249,165-record
    table at 1 and 3 CUs between two default-grid calls, under a max_length
    that cuts the reply inside its last tenth.

    A present hash sends one 87-byte part (12 + key count, one cumulative
    length, 8 key bytes, 64 value bytes), an absent one nothing.  The grids are
    capped at 8 workgroups of 256 lanes per CU: at 1 CU 8 workgroups take 977
    tiles of 256 hashes in 123 passes, at 3 CUs 24 workgroups in 41; the scan's
    one workgroup takes the 977 tile sums in two steps of 512 and then the tile
    the reply ends in, hash by hash; the gather's tiles behind that one write
    only d_parts."""
    ws, key_cap, kb, q, looked = grid_case
    nq = q.shape[0]
    hit = looked["kind"] == lc.OBJECT
    keys = kb.view("<u8")
    assert (q["table_id"][hit] == 0).all() and hit.sum() == nq // 2
    hashes = np.array([pc.key_hash(0, int(k if h else k + (1 << 40)).to_bytes(8, "little"))
                       for k, h in zip(keys.tolist(), hit.tolist())], np.uint64)
    size = np.where(hit, 87, 0).astype(np.int64)
    ends = np.cumsum(size)
    starts = ends - size
    ml = int(starts[nq * 19 // 20]) + 7
    n = int((starts <= ml).sum())
    assert nq * 9 // 10 < n < nq and n % 256 not in (0, 255)
    cap = ml + 87   # max_length and the longest hash's parts: the reference's rule alone decides
    want_parts = np.zeros(nq, rh.PART)
    want_parts["off"] = np.where(np.arange(nq) < n, starts, rh.NONE).astype(np.uint64)
    want_parts["objects"] = np.where(np.arange(nq) < n, hit, 0)
    h = np.flatnonzero(hit[:n])
    hdr = np.zeros(h.size, segments.READ_HASHES_OBJECT_DTYPE)
    hdr["version"] = looked["version"][h]
    hdr["length"] = 75
    want = np.zeros(int(ends[n - 1]), np.uint8)
    want[starts[h, None] + np.arange(12)] = hdr.view(np.uint8).reshape(h.size, 12)
    src = looked["segment"][h].astype(np.int64) * ws[0].cap + looked["value_off"][h] - 11
    want[starts[h, None] + 12 + np.arange(75)] = ws[0].buf[src[:, None] + np.arange(75)]
    summary = dict(rh.ZERO_SUMMARY, hashes=n, objects=h.size, objects_counted=h.size + int(hit[n]),
                   reply_bytes=int(ends[n - 1]), value_bytes=64 * h.size, key_bytes=11 * h.size,
                   empty=n - h.size)
    assert cap >= want.size
    c = ramcrc.Context(0)
    t = None
    try:
        t = ramcrc.ReplayTable(c, key_cap, 2)
        for a in [tc.Added(w) for w in ws]:
            a.add(t)
        for ncu in (0, 1, 3, 0):
            c.set_cus(ncu)   # 0: every CU again
            g = rh.Asked(c, t, 0, hashes, cap, cap, ml)
            assert g.summary == summary, ("grid", ncu, g.summary)
            assert np.array_equal(g.reply_all[:want.size], want), ("grid", ncu)
            assert lc.same(g.parts, want_parts), ("grid", ncu)
    finally:
        if t is not None:
            t.close()
        c.close()


# ----------------------------------------------------------- spoiled tables
def test_spoiled_tables(ramcrc, oracle_mod):
    """Spoiled by a bad segment number and by the key capacity: the pre-filled
    reply and parts stay untouched, the summary is zero with spoiled = 1, the
    call raises no refusal of its own, and after the reset the table answers
    again."""
    c = ramcrc.Context(0)
    drv = rh.DeviceDriver(ramcrc, oracle_mod, c)
    try:
        b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad.d_entries[2, 0] = 1   # = n_seg
        full = drv.batch([tc.capacity_lists(64)])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        for first, spoiler, tid, key in ((b, bad, 1, b"y"), (full, more, 7, b"cap key 3")):
            asked = [rh.key_hash((tid, key)), 5]
            tab = drv.table(64, 4)
            try:
                tab.add(first)
                g, _ = rh.ask(tab, rh.checked(tab), rh.key_hash, tid, asked, what="before")
                assert g.summary["objects"] == 1
                tc.Added(spoiler).add(tab.t)
                with pytest.raises(ramcrc.RamcrcError) as e:
                    c.check()
                assert e.value.code == ramcrc.EREFUSED
                for want_parts in (True, False):
                    g = rh.Asked(c, tab.t, tid, asked, 256, 256, rh.HUGE, want_parts=want_parts)   # check() passes
                    assert g.summary == rh.SPOILED_SUMMARY and (g.reply_all == FILL).all()
                    assert g.parts_all is None or (g.parts_all == FILL).all()
                tab.reset()
                tab.add(first)
                rh.ask(tab, rh.checked(tab), rh.key_hash, tid, asked, what="after the reset")
            finally:
                tab.close()
    finally:
        c.close()


# ---------------------------------------------------------------- the chain
def test_chain(ctx, ramcrc, drv):
    """verify -> two adds with the partition call's hashes -> read_hashes ->
    read_hashes_objects on the host: every hash carries what the test wrote for
    the key's newest object."""
    rng = np.random.default_rng(47)
    newest, lists = {}, [[tc.head(1)], [tc.head(2)], [tc.head(3)], [tc.head(4)]]
    for n in range(120):
        key = (1, b"chain key %d" % n)
        for ver in (1 + rng.permutation(4)[:int(rng.integers(1, 4))]).tolist():
            value = rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
            lists[int(rng.integers(0, 4))].append(rc.obj(key[0], key[1], ver, value))
            if key not in newest or ver > newest[key][0]:
                newest[key] = (ver, value)
    dead = (1, b"chain key 7")
    lists[3].append(rc.tomb(dead[0], dead[1], 9))
    ws = [drv.batch(lists[:2]), drv.batch(lists[2:])]
    tabs = pc.tablets([(1, 0, tc.ALL, 0, 0, 0)])
    t = ramcrc.ReplayTable(ctx, 1000, 2)
    try:
        for w in ws:
            crc = torch.zeros(w.d_entries.shape[0], dtype=torch.int32, device="cuda")
            ctx.verify_objects(w.d, w.cap, w.d_entries, w.d_n, crc, w.d_status.clone())
            h = drv.ramcrc.recovery_partition_host(w.buf, w.cap, w.nseg, w.status, w.table, tabs, 1)[2]
            tc.Added(w, np.asarray(h, np.uint64)[:w.table.shape[0]]).add(t)
        keys = sorted(newest)
        asked = [rh.key_hash(k) for k in keys]
        g = rh.Asked(ctx, t, 1, asked, 1 << 20, 1 << 20, rh.HUGE)
        objs = segments.read_hashes_objects(g.reply, g.summary["objects"])
        assert g.summary["hashes"] == len(keys) and g.summary["objects"] == 119 == len(objs)
        assert g.summary["tombstones"] == 1 and g.summary["empty"] == 1
        live = [k for k in keys if k != dead]
        for key, (version, data) in zip(live, objs):
            ver, value = newest[key]
            assert (version, data) == (ver, b"\1" + len(key[1]).to_bytes(2, "little") + key[1] + value), key
        assert g.summary["value_bytes"] == sum(len(newest[k][1]) for k in live)
        assert tuple(int(x) for x in g.parts[keys.index(dead)])[1:] == (0, 0)
    finally:
        t.close()


def test_bad_arguments(ctx, ramcrc):
    """Any flag, missing arrays and misaligned arrays are EINVAL before any
    launch: nothing is written and the context stays clean."""
    t = ramcrc.ReplayTable(ctx, 64, 1)
    try:
        z = torch.full((512,), FILL, dtype=torch.uint8, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()
        good = dict(hashes=z[:8], n=1, flags=0, reply=z[64:128], cap=64, parts=z[128:144], summary=z[192:264])
        assert all(p(good[k]) % 16 == 0 for k in ("hashes", "parts", "summary"))
        cases = [dict(flags=1), dict(flags=1 << 31), dict(summary=None), dict(hashes=None), dict(reply=None),
                 dict(hashes=z[4:12]), dict(parts=z[132:148]), dict(summary=z[196:268]),
                 dict(n=0xFFFFFFFF), dict(summary=None, n=0, hashes=None)]
        for change in cases:
            a = dict(good, **change)
            with pytest.raises(ramcrc.RamcrcError) as e:
                ramcrc._check(ramcrc.lib().ramcrc_replay_table_read_hashes_device(
                    t._h, 1, p(a["hashes"]), a["n"], a["flags"], p(a["reply"]), a["cap"], 64, p(a["parts"]),
                    p(a["summary"]), None), "read_hashes")
            assert e.value.code == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
    finally:
        t.close()


def test_the_call_does_not_allocate_after_reserve(ctx, ramcrc, drv):
    """After ramcrc_ctx_reserve(ctx, 32 + 16 * ceil(n / 256), 6 * n) a call of n
    hashes takes no scratch, as the header states."""
    tab, hash_of = rh.truncation_table(drv)
    c2 = ramcrc.Context(0)   # a context that has reserved nothing yet
    t2 = ramcrc.ReplayTable(c2, 64, 1)
    try:
        n = 3000
        a = tab.added[0]
        tc.Added(a.w, a.d_hash).add(t2)
        c2.reserve(32 + 16 * -(-n // 256), 6 * n)
        before = ramcrc.scratch_allocations()
        g = rh.Asked(c2, t2, 1, [105, 60, 999] * (n // 3), n * 64, n * 64, rh.HUGE)
        assert ramcrc.scratch_allocations() == before
        assert g.summary["hashes"] == n and g.summary["objects"] == 4 * (n // 3)
    finally:
        t2.close()
        c2.close()
        tab.close()
