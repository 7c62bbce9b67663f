"""ramcrc_replay_table_write_device: a multi-write against the replay table on
the GPU (k_wr_group, k_wr_size, k_wr_scan, k_wr_emit), the loop of
MasterService::multiWrite (src/MasterService.cc:1523-1601) over
ObjectManager::writeObject (src/ObjectManager.cc:1181-1350).

The scenarios are write_cases.py's, the ones test_replay_table_write_host.py
runs on the host: every batch is walked by ctx.segment_walk, the expectation
(plain Python, held against the goldens and the live query's winners) is what
every device write is held against, a host table fed the same batches must
give the same bytes, and the output, walked with the call's certificate by
ramcrc_replay_verify_device, is added as the next batch.  Every output is
pre-filled with 0xA5 and checked past its end."""
import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import replay_table_cases as tc
import resolve_cases as rc
import write_cases as wc
from append_cases import Walked
from test_gpu_replay_table_lookup import grid_case  # noqa: F401  (the 249,165-record table)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = wc.FILL


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return wc.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_goldens(drv, oracle_mod):
    ref = wc.golden()
    assert wc.check_expectation_against_golden(oracle_mod, ref) == ref["steps"]
    wc.case_goldens(drv)


def test_closing_the_loop(drv, mixed):
    wc.case_closing_the_loop(drv, mixed)


def test_reject_rules(drv):
    wc.case_reject_rules(drv)


def test_versions(drv):
    wc.case_versions(drv)


def test_duplicates(drv):
    wc.case_duplicates(drv)


def test_entry_sizes(drv):
    wc.case_sizes(drv)


def test_alignment(drv):
    wc.case_alignment(drv)


def test_multi_key_objects(drv):
    wc.case_multi_key(drv)


def test_space(drv):
    wc.case_space(drv)


def test_bad_requests_and_bad_rules_among_good_ones(drv):
    wc.case_bad_requests(drv)


def test_nullable_and_empty_arguments(drv):
    wc.case_nullable_and_empty(drv)


def test_read_only(drv, mixed):
    wc.case_read_only(drv, mixed)


# --------------------------------------------------------------- grid size
def test_small_grids(ramcrc, oracle_mod, grid_case):  # noqa: F811
    """250,000 requests against the 249,165-record table (and the batch a first
    write adds to it) at 1 and 3 CUs between two default-grid calls: every
    second one overwrites a key, the others are new keys, every 97th repeats
    the request before it, and the capacity cuts the output inside its last
    tenth.

    An overwrite is a 101-byte object entry (24 + key count, one cumulative
    length, 8 key bytes, 64 value bytes) and a 42-byte tombstone entry, a new
    key the object alone.  The grids are capped at 8 workgroups of 256 lanes
    per CU: at 1 CU 8 workgroups take 977 tiles of 256 requests in 123 passes,
    at 3 CUs 24 workgroups in 41; the scan's one workgroup takes the 977 tile
    sums in four steps of 256 and then the tile the output ends in, request by
    request; the emit's tiles behind that one write only parts and references."""
    ws, key_cap, kb, q, _ = grid_case
    nq = q.shape[0]
    i = np.arange(nq)
    dup = i % 97 == 96
    src = np.where(dup, i - 1, i)
    rng = np.random.default_rng(31)
    data = np.zeros((nq, 75), np.uint8)
    data[:, 0], data[:, 1] = 1, 8
    data[:, 3:11] = kb.reshape(nq, 8)[src]
    data[:, 11:] = rng.integers(0, 256, (nq, 64), dtype=np.uint8)
    reqs = np.zeros(nq, wc.REQ)
    reqs["table_id"], reqs["data_off"], reqs["data_len"] = q["table_id"][src], 75 * i, 75
    look = np.zeros(nq, lc.KEY)
    look["table_id"], look["key_off"], look["key_len"] = reqs["table_id"], 75 * i + 3, 8
    seg_ids = np.array([500, 900, 1300], np.uint64)
    nv = 1 << 33
    c = ramcrc.Context(0)
    tab = None
    try:
        drv = wc.DeviceDriver(ramcrc, oracle_mod, c)
        tab = wc.DeviceTab(drv, key_cap, 3)
        for w in ws:
            tab.add(w)
        # The table's objects have version 0, VERSION_NONEXISTENT to a write.  A
        # first write gives the keys of batch 0 versions from 7 on; its output,
        # walked and added, holds the objects the second write replaces.
        a = np.flatnonzero((i % 2 == 0) & ~dup)
        room = 101 * a.size
        g = wc.Written(c, tab.t, data.reshape(-1), reqs[a], room, room, 7, wc.TS)
        wc._check_got(g, a.size, room)
        assert g.summary["ok"] == g.summary["allocated"] == a.size and g.summary["out_bytes"] == room
        assert np.array_equal(g.parts["version"], 7 + np.arange(a.size, dtype=np.uint64))
        cap_a = -(-room // 16) * 16
        buf = np.zeros(cap_a, np.uint8)
        buf[:room] = np.frombuffer(g.out, np.uint8)
        wa = Walked(c, buf, np.array([g.cert], np.uint32), cap_a, 1, min_entry=64)
        assert int(wa.status[0, 0]) == segments.SEG_OK and wa.table.shape[0] == a.size
        tab.add(wa)
        looked, _ = tab.twin.lookup(data.reshape(-1), look)
        hit = looked["kind"] == lc.OBJECT
        cur = np.where(hit, looked["version"], 0).astype(np.uint64)
        assert hit[a].all() and (looked["batch"][a] == 2).all() and (cur[a] >= 7).all() and hit.sum() > nq * 0.49
        hit &= cur != 0

        served = ~dup
        size = np.where(served, np.where(hit, 101 + 42, 101), 0).astype(np.int64)
        ends = np.cumsum(size)
        cap = int(ends[nq * 19 // 20]) + 7
        fits = served & (ends <= cap)
        first_out = int(np.flatnonzero(served & ~fits)[0])
        # the cut falls inside a tile, not on its edge
        assert nq * 9 // 10 < first_out < nq and first_out % 256 not in (0, 255)
        alloc = served & ~hit
        version = np.where(hit, cur + np.uint64(1), np.uint64(nv) + (np.cumsum(alloc) - alloc).astype(np.uint64))
        parts = np.zeros(nq, wc.PART)
        parts["status"] = np.where(fits, wc.OK, wc.RETRY)
        parts["version"] = np.where(fits, version, np.where(dup, np.uint64(0), cur))
        refs = np.zeros(nq, wc.REF)
        refs["object_off"] = np.where(fits, ends - size, wc.NONE)
        refs["tombstone_off"] = np.where(fits & hit, ends - 42, wc.NONE)
        head = int(ends[fits][-1])
        n_ok, n_tomb = int(fits.sum()), int((fits & hit).sum())
        summary = dict(dict.fromkeys(wc.SUMMARY_NAMES, 0), ok=n_ok, retry_duplicate=int(dup.sum()),
                       retry_full=int((served & ~fits).sum()), tombstones=n_tomb, allocated=int(alloc.sum()),
                       next_version=nv + int(alloc.sum()), out_bytes=head, value_bytes=64 * n_ok,
                       key_bytes=11 * n_ok, object_bytes=99 * n_ok, tombstone_bytes=40 * n_tomb)
        assert n_tomb > nq // 3
        first = None
        for ncu in (0, 1, 3, 0):
            c.set_cus(ncu)   # 0: every CU again
            g = wc.Written(c, tab.t, data.reshape(-1), reqs, cap, cap, nv, wc.TS, seg_ids=seg_ids)
            wc._check_got(g, nq, cap)
            assert g.summary == summary, ("grid", ncu, g.summary, summary)
            assert lc.same(g.parts, parts) and lc.same(g.refs, refs) and lc.same(g.old, looked), ("grid", ncu)
            if first is None:
                first = g
                # once: the host twin's bytes, and the device's own walk and checksum pass
                h = tab.host.write_raw(data.reshape(-1), reqs, cap, nv, wc.TS, seg_ids=seg_ids, room=cap)
                assert h.out == g.out and h.cert == g.cert and h.summary == g.summary
                cap16 = -(-cap // 16) * 16
                d = torch.zeros(cap16, dtype=torch.uint8, device="cuda")
                d[:head] = g.d_out[:head]
                dc = torch.from_numpy(np.array([g.cert], np.uint32).view(np.int32)).cuda()
                st = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
                ent = torch.zeros((n_ok + n_tomb + 8, 4), dtype=torch.int32, device="cuda")
                dn = torch.zeros(1, dtype=torch.int64, device="cuda")
                crc = torch.zeros(n_ok + n_tomb + 8, dtype=torch.int32, device="cuda")
                c.replay_verify(d, cap16, cap16, 1, dc, st, ent, dn, crc)
                c.check()
                st = st.cpu().numpy().view(np.uint32)[0]
                assert int(st[0]) == segments.SEG_OK and int(st[2]) == n_ok + n_tomb == int(dn.item())
                assert int(st[3]) == 0
            else:
                assert g.out == first.out and g.cert == first.cert, ("grid", ncu)
    finally:
        if tab is not None:
            tab.close()
        c.close()


# ----------------------------------------------------------- spoiled tables
def test_a_spoiled_table(ramcrc, oracle_mod):
    """Spoiled by the key capacity: every pre-filled output but the summary
    stays untouched, the summary is zero with spoiled = 1, the write raises no
    refusal of its own, and after the reset the table takes writes again."""
    c = ramcrc.Context(0)
    drv = wc.DeviceDriver(ramcrc, oracle_mod, c)
    objs = [(7, b"cap key 3", b"new"), (1, b"fresh", b"f")]
    data, reqs = segments.write_requests(objs)
    try:
        full = drv.batch([tc.capacity_lists(64)])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        tab = drv.table(64, 4)
        try:
            tab.add(full)
            wc.write(tab, wc.checked(tab), objs, what="before")
            tc.Added(more).add(tab.t)
            with pytest.raises(ramcrc.RamcrcError) as e:
                c.check()
            assert e.value.code == ramcrc.EREFUSED
            for kw in (dict(), dict(want_refs=False, want_old=False)):
                g = wc.Written(c, tab.t, data, reqs, 4096, 4096, **kw)   # its check() passes: nothing is refused anew
                assert g.summary == wc.SPOILED_SUMMARY and (g.summary_past == FILL).all()
                for a in (g.out_all, g.parts, g.parts_past, g.cert_past, g.refs, g.old):
                    assert a is None or (np.ascontiguousarray(a).view(np.uint8) == FILL).all()
                assert g.cert == (wc.FILL32, wc.FILL32)
            tab.reset()
            tab.add(full)
            wc.write(tab, wc.checked(tab), objs, what="after the reset")
        finally:
            tab.close()
    finally:
        c.close()


def test_bad_arguments(ctx, ramcrc):
    """Missing arrays, misaligned arrays and next_version = 0 are EINVAL before
    any launch: nothing is written and the context stays clean."""
    t = ramcrc.ReplayTable(ctx, 64, 1)
    try:
        z = torch.full((1024,), FILL, dtype=torch.uint8, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()
        good = dict(data=z[:16], reqs=z[32:56], hashes=z[64:72], rules=z[80:96], nv=1, seg=z[96:104], out=z[112:176],
                    cap=64, cert=z[176:184], parts=z[192:204], refs=z[208:216], old=z[224:256], summary=z[256:384])
        assert all(p(v) % 16 == 0 for k, v in good.items() if k not in ("nv", "cap"))
        cases = [dict(nv=0), dict(summary=None), dict(cert=None), dict(reqs=None), dict(parts=None), dict(out=None),
                 dict(data=None), dict(reqs=z[36:60]), dict(hashes=z[68:76]), dict(rules=z[84:100]),
                 dict(seg=z[100:108]), dict(cert=z[178:186]), dict(parts=z[194:206]), dict(refs=z[212:220]),
                 dict(old=z[232:264]), dict(summary=z[260:388])]
        for change in cases:
            a = dict(good, **change)
            with pytest.raises(ramcrc.RamcrcError) as e:
                ramcrc._check(ramcrc.lib().ramcrc_replay_table_write_device(
                    t._h, p(a["data"]), 16, p(a["reqs"]), 1, p(a["hashes"]), p(a["rules"]), a["nv"], 0, p(a["seg"]),
                    p(a["out"]), a["cap"], p(a["cert"]), p(a["parts"]), p(a["refs"]), p(a["old"]), p(a["summary"]),
                    None), "write")
            assert e.value.code == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
    finally:
        t.close()
