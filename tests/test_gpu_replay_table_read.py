"""ramcrc_replay_table_read_device: a multi-read's reply packed on the GPU
(k_rtab_read_size, k_rtab_read_scan, k_rtab_read_gather), the loop of
MasterService::multiRead (src/MasterService.cc:1352-1415) over readObject and
rejectOperation (src/ObjectManager.cc:324-369, :2893-2907).

The scenarios are read_cases.py's, the ones test_replay_table_read_host.py runs
on the host: every batch is walked by ctx.segment_walk, the expectation (plain
Python, held against the goldens and the live query's winners) is what every
device read is held against, and a host table fed the same batches must give
the same bytes.  Reply, part offsets, results and summary are pre-filled with
0xA5 and checked past their ends."""
import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import read_cases as rd
import replay_table_cases as tc
import resolve_cases as rc
from test_gpu_replay_table_lookup import grid_case  # noqa: F401  (the 249,165-record table)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = rd.FILL


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return rd.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_goldens(drv):
    assert rd.check_expectation_against_golden(rd.golden()) == 9
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


# --------------------------------------------------------------- grid size
def test_small_grids(ramcrc, grid_case):  # noqa: F811
    """250,000 queries, half hits and half misses, against the 249,165-record
    table at 1 and 3 CUs between two default-grid calls, under a limit that
    cuts the reply inside its last tenth.

    A hit is a 91-byte part (16 + key count, one cumulative length, 8 key
    bytes, 64 value bytes), a miss a 16-byte one.  The grids are capped at 8
    workgroups of 256 lanes per CU: at 1 CU 8 workgroups take 977 tiles of 256
    queries in 123 passes, at 3 CUs 24 workgroups in 41; the scan's one
    workgroup takes the 977 tile sums in two steps of 512 and then the tile the
    reply ends in, query by query; the gather's tiles behind that one write
    only d_part_off."""
    ws, key_cap, kb, q, looked = grid_case
    nq = q.shape[0]
    hit = looked["kind"] == lc.OBJECT
    size = np.where(hit, 91, 16).astype(np.int64)
    ends = np.cumsum(size)
    cap = int(ends[nq * 19 // 20]) + 7
    n = int((ends <= cap).sum())
    assert nq * 9 // 10 < n < nq and n % 256 not in (0, 255)
    off = ends - size
    want_off = np.where(np.arange(nq) < n, off, rd.NONE).astype(np.uint64)
    hdr = np.zeros(n, segments.READ_PART_DTYPE)
    hdr["status"] = np.where(hit[:n], rd.OK, rd.DOESNT_EXIST)
    hdr["version"] = np.where(hit[:n], looked["version"][:n], 0)
    hdr["length"] = np.where(hit[:n], 75, 0)
    want = np.zeros(int(ends[n - 1]), np.uint8)
    want[off[:n, None] + np.arange(16)] = hdr.view(np.uint8).reshape(n, 16)
    h = np.flatnonzero(hit[:n])
    src = looked["segment"][h].astype(np.int64) * ws[0].cap + looked["value_off"][h] - 11
    want[off[h, None] + 16 + np.arange(75)] = ws[0].buf[src[:, None] + np.arange(75)]
    summary = dict(dict.fromkeys(rd.SUMMARY_NAMES, 0), returned=n, reply_bytes=int(ends[n - 1]), ok=h.size,
                   doesnt_exist=n - h.size, value_bytes=64 * h.size, key_bytes=11 * h.size)
    c = ramcrc.Context(0)
    t = None
    try:
        t = ramcrc.ReplayTable(c, key_cap, 2)
        for a in [tc.Added(w) for w in ws]:
            a.add(t)
        for ncu in (0, 1, 3, 0):
            c.set_cus(ncu)   # 0: every CU again
            g = rd.Read(c, t, kb, q, cap, cap)
            assert g.summary == summary, ("grid", ncu, g.summary)
            assert np.array_equal(g.reply_all[:want.size], want), ("grid", ncu)
            rd._check_got(g, nq, True, True)
            assert np.array_equal(g.off, want_off) and lc.same(g.results, looked), ("grid", ncu)
    finally:
        if t is not None:
            t.close()
        c.close()


# ----------------------------------------------------------- spoiled tables
def test_spoiled_tables(ramcrc, oracle_mod):
    """Spoiled by a bad segment number and by the key capacity: the pre-filled
    reply, part offsets and results stay untouched, the summary is zero with
    spoiled = 1, the read raises no refusal of its own, and after the reset
    the table answers again."""
    c = ramcrc.Context(0)
    drv = rd.DeviceDriver(ramcrc, oracle_mod, c)
    keys = [(1, b"x"), (7, b"cap key 3"), (1, b"absent"), (1, b"y")]
    kb, q = segments.lookup_queries(keys)
    try:
        b = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad = drv.batch([[tc.head(1)] + rc.tiny_entries()])
        bad.d_entries[2, 0] = 1   # = n_seg
        full = drv.batch([tc.capacity_lists(64)])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        for first, spoiler in ((b, bad), (full, more)):
            tab = drv.table(64, 4)
            try:
                tab.add(first)
                rd.read(tab, rd.checked(tab), keys, what="before")
                tc.Added(spoiler).add(tab.t)
                with pytest.raises(ramcrc.RamcrcError) as e:
                    c.check()
                assert e.value.code == ramcrc.EREFUSED
                for kw in (dict(), dict(want_off=False, want_res=False)):
                    g = rd.Read(c, tab.t, kb, q, 4096, 4096, **kw)   # its check() passes: nothing is refused anew
                    assert g.summary == rd.SPOILED_SUMMARY and (g.summary_past == rd.FILL32).all()
                    assert (g.reply_all == FILL).all()
                    assert g.off_all is None or (g.off_all == rd.FILL64).all()
                    assert g.res_all is None or (g.res_all == FILL).all()
                tab.reset()
                tab.add(first)
                rd.read(tab, rd.checked(tab), keys, what="after the reset")
            finally:
                tab.close()
    finally:
        c.close()


# ---------------------------------------------------------------- the chain
def test_chain(ctx, ramcrc, drv):
    """verify -> two adds -> read -> multi_read_parts on the host: every part
    carries what the test wrote for the key's newest object."""
    rng = np.random.default_rng(43)
    newest, lists = {}, [[tc.head(1)], [tc.head(2)], [tc.head(3)], [tc.head(4)]]
    for n in range(120):
        key = (1 + n % 3, b"chain key %d" % n)
        for ver in (1 + rng.permutation(4)[:int(rng.integers(1, 4))]).tolist():
            value = rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
            lists[int(rng.integers(0, 4))].append(rc.obj(key[0], key[1], ver, value))
            if key not in newest or ver > newest[key][0]:
                newest[key] = (ver, value)
    dead = (2, b"chain key 7")
    lists[3].append(rc.tomb(dead[0], dead[1], 9))
    ws = [drv.batch(lists[:2]), drv.batch(lists[2:])]
    t = ramcrc.ReplayTable(ctx, 1000, 2)
    try:
        for w in ws:
            crc = torch.zeros(w.d_entries.shape[0], dtype=torch.int32, device="cuda")
            ctx.verify_objects(w.d, w.cap, w.d_entries, w.d_n, crc, w.d_status.clone())
            tc.Added(w).add(t)
        keys = sorted(newest)
        kb, q = segments.lookup_queries(keys)
        for value_only in (True, False):
            g = rd.Read(ctx, t, kb, q, 1 << 20, 1 << 20, value_only=value_only)
            parts = segments.multi_read_parts(g.reply, g.summary["returned"])
            assert len(parts) == len(keys) == g.summary["returned"]
            for key, (status, version, data) in zip(keys, parts):
                if key == dead:
                    assert (status, version, data) == (rd.DOESNT_EXIST, 0, b"")
                    continue
                ver, value = newest[key]
                head = b"" if value_only else b"\1" + len(key[1]).to_bytes(2, "little") + key[1]
                assert (status, version, data) == (rd.OK, ver, head + value), key
            assert g.summary["ok"] == 119 and g.summary["doesnt_exist"] == 1
            assert g.summary["value_bytes"] == sum(len(v) for k, (_, v) in newest.items() if k != dead)
    finally:
        t.close()


def test_bad_arguments(ctx, ramcrc):
    """Unknown flags, missing arrays and misaligned arrays are EINVAL before
    any launch: nothing is written and the context stays clean."""
    t = ramcrc.ReplayTable(ctx, 64, 1)
    try:
        z = torch.full((512,), FILL, dtype=torch.uint8, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()
        good = dict(queries=z[:24], rules=z[32:48], flags=0, reply=z[64:128], cap=64, part_off=z[128:136],
                    results=z[144:176], summary=z[192:272])
        assert all(p(good[k]) % 16 == 0 for k in ("queries", "rules", "part_off", "results", "summary"))
        cases = [dict(flags=2), dict(flags=1 << 31), dict(summary=None), dict(queries=None), dict(reply=None),
                 dict(queries=z[4:28]), dict(rules=z[36:52]), dict(results=z[152:184]),
                 dict(part_off=z[132:140]), dict(summary=z[196:276])]
        for change in cases:
            a = dict(good, **change)
            with pytest.raises(ramcrc.RamcrcError) as e:
                ramcrc._check(ramcrc.lib().ramcrc_replay_table_read_device(
                    t._h, None, 0, p(a["queries"]), 1, None, p(a["rules"]), a["flags"], p(a["reply"]), a["cap"],
                    p(a["part_off"]), p(a["results"]), p(a["summary"]), None), "read")
            assert e.value.code == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
    finally:
        t.close()
