"""ramcrc_replay_table_remove_device: a multi-remove against the replay table
on the GPU (k_rm_group, k_rm_size, k_rm_scan, k_rm_emit), the loop of
MasterService::multiRemove (src/MasterService.cc:1435-1505) over
ObjectManager::removeObject (src/ObjectManager.cc:405-491).

The scenarios are remove_cases.py's, the ones test_replay_table_remove_host.py
runs on the host: every batch is walked by ctx.segment_walk, the expectation
(plain Python, held against the goldens and the live query's winners) is what
every device remove is held against, a host table fed the same batches must
give the same bytes, and the output, walked with the call's certificate by
ramcrc_replay_verify_device, is added as the next batch.  Every output is
pre-filled with 0xA5 and checked past its end."""
import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import remove_cases as rm
import replay_table_cases as tc
import resolve_cases as rc
from test_gpu_replay_table_lookup import grid_case  # noqa: F401  (the 249,165-record table)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = rm.FILL


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return rm.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_goldens(drv, oracle_mod):
    ref = rm.golden()
    assert rm.check_expectation_against_golden(oracle_mod, ref) == ref["steps"]
    rm.case_goldens(drv)


def test_closing_the_loop(drv, mixed):
    rm.case_closing_the_loop(drv, mixed)


def test_reject_rules(drv):
    rm.case_reject_rules(drv)


def test_version_zero(drv):
    rm.case_version_zero(drv)


def test_duplicates(drv):
    rm.case_duplicates(drv)


def test_key_lengths(drv):
    rm.case_key_lengths(drv)


def test_alignment(drv):
    rm.case_alignment(drv)


def test_space(drv):
    rm.case_space(drv)


def test_counts(drv):
    rm.case_counts(drv)


def test_bad_requests_and_bad_rules_among_good_ones(drv):
    rm.case_bad_requests(drv)


def test_nullable_arguments(drv):
    rm.case_nullable(drv)


def test_read_only(drv, mixed):
    rm.case_read_only(drv, mixed)


# --------------------------------------------------------------- grid size
def test_small_grids(ramcrc, oracle_mod, grid_case):  # noqa: F811
    """250,000 requests against the 249,165-record table at 1 and 3 CUs
    between two default-grid calls: every second one a present key, the others
    absent, every 97th a repeat of the request before it, and the capacity
    cuts the output inside its last tenth.

    A removed key is one 42-byte tombstone entry (two metadata bytes, the
    32-byte header, 8 key bytes): the lane class.  The grids are capped at 8
    workgroups of 256 lanes per CU: at 1 CU 8 workgroups take 977 tiles of 256
    requests in 123 passes, at 3 CUs 24 workgroups in 41; the scan's one
    workgroup takes the 977 tile sums in four steps of 256 and then the tile
    the output ends in, request by request; the emit's tiles behind that one
    write only parts and references."""
    ws, key_cap, kb, q, want = grid_case
    nq = q.shape[0]
    i = np.arange(nq)
    dup = i % 97 == 96
    src = np.where(dup, i - 1, i)
    reqs = q[src].copy()
    looked = want[src].copy()
    hit = looked["kind"] == lc.OBJECT
    cur = np.where(hit, looked["version"], 0).astype(np.uint64)
    served = ~dup
    reach = served & hit
    size = np.where(reach, 42, 0).astype(np.int64)
    ends = np.cumsum(size)
    cap = int(ends[nq * 19 // 20]) + 7
    fits = reach & (ends <= cap)
    first_out = int(np.flatnonzero(reach & ~fits)[0])
    # the cut falls inside a tile, not on its edge
    assert nq * 9 // 10 < first_out < nq and first_out % 256 not in (0, 255)
    nv = 1 << 33
    parts = np.zeros(nq, rm.PART)
    parts["status"] = np.where(dup | (reach & ~fits), rm.RETRY, rm.OK)
    parts["version"] = np.where(reach, cur, np.uint64(0))
    refs = np.where(fits, ends - 42, rm.NONE).astype(np.uint32)
    head = int(ends[fits][-1])
    n_rm = int(fits.sum())
    summary = dict(dict.fromkeys(rm.SUMMARY_NAMES, 0), removed=n_rm, ok_absent=int((served & ~hit).sum()),
                   retry_duplicate=int(dup.sum()), retry_full=int((reach & ~fits).sum()),
                   next_version=max(nv, int(cur[fits].max()) + 1), out_bytes=head, tombstone_bytes=40 * n_rm)
    assert n_rm > nq // 3 and summary["retry_full"] > 0
    seg_ids = np.array([500, 900], np.uint64)
    c = ramcrc.Context(0)
    tab = None
    try:
        drv = rm.DeviceDriver(ramcrc, oracle_mod, c)
        tab = rm.DeviceTab(drv, key_cap, 2)
        for w in ws:
            tab.add(w)
        first = None
        for ncu in (0, 1, 3, 0):
            c.set_cus(ncu)   # 0: every CU again
            g = rm.Removed(c, tab.t, kb, reqs, cap, cap, nv, rm.TS, seg_ids=seg_ids)
            rm._check_got(g, nq, cap)
            assert g.summary == summary, ("grid", ncu, g.summary, summary)
            assert lc.same(g.parts, parts) and lc.same(g.refs, refs) and lc.same(g.old, looked), ("grid", ncu)
            if first is None:
                first = g
                # once: the host twin's bytes, and the device's own walk and checksum pass
                h = tab.host.remove_raw(kb, reqs, cap, nv, rm.TS, seg_ids=seg_ids, room=cap)
                assert h.out == g.out and h.cert == g.cert and h.summary == g.summary
                assert lc.same(h.parts, g.parts) and lc.same(h.refs, g.refs) and lc.same(h.old, g.old)
                cap16 = -(-cap // 16) * 16
                d = torch.zeros(cap16, dtype=torch.uint8, device="cuda")
                d[:head] = g.d_out[:head]
                dc = torch.from_numpy(np.array([g.cert], np.uint32).view(np.int32)).cuda()
                st = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
                ent = torch.zeros((n_rm + 8, 4), dtype=torch.int32, device="cuda")
                dn = torch.zeros(1, dtype=torch.int64, device="cuda")
                crc = torch.zeros(n_rm + 8, dtype=torch.int32, device="cuda")
                c.replay_verify(d, cap16, cap16, 1, dc, st, ent, dn, crc)
                c.check()
                st = st.cpu().numpy().view(np.uint32)[0]
                assert int(st[0]) == segments.SEG_OK and int(st[2]) == n_rm == int(dn.item())
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
    stays untouched, the summary is zero with spoiled = 1, the remove raises no
    refusal of its own, and after the reset the table takes removes again."""
    c = ramcrc.Context(0)
    drv = rm.DeviceDriver(ramcrc, oracle_mod, c)
    keys = [(7, b"cap key 3"), (1, b"fresh")]
    kb, reqs = segments.lookup_queries(keys)
    try:
        full = drv.batch([tc.capacity_lists(64)])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        tab = drv.table(64, 4)
        try:
            tab.add(full)
            g, w = rm.remove(tab, rm.checked(tab), keys, what="before")
            assert w.summary["removed"] == 1
            tc.Added(more).add(tab.t)
            with pytest.raises(ramcrc.RamcrcError) as e:
                c.check()
            assert e.value.code == ramcrc.EREFUSED
            for kw in (dict(), dict(want_refs=False, want_old=False)):
                g = rm.Removed(c, tab.t, kb, reqs, 4096, 4096, **kw)   # its check() passes: nothing is refused anew
                assert g.summary == rm.SPOILED_SUMMARY and (g.summary_past == FILL).all()
                for a in (g.out_all, g.parts, g.parts_past, g.cert_past, g.refs, g.old):
                    assert a is None or (np.ascontiguousarray(a).view(np.uint8) == FILL).all()
                assert g.cert == (rm.FILL32, rm.FILL32)
            tab.reset()
            tab.add(full)
            rm.remove(tab, rm.checked(tab), keys, what="after the reset")
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
        good = dict(keys=z[:16], reqs=z[32:56], hashes=z[64:72], rules=z[80:96], nv=1, seg=z[96:104], out=z[112:176],
                    cap=64, cert=z[176:184], parts=z[192:204], refs=z[208:212], old=z[224:256], summary=z[256:352],
                    n=1)
        assert all(p(v) % 16 == 0 for k, v in good.items() if k not in ("nv", "cap", "n"))
        cases = [dict(nv=0), dict(summary=None), dict(cert=None), dict(reqs=None), dict(parts=None), dict(out=None),
                 dict(keys=None), dict(reqs=z[36:60]), dict(hashes=z[68:76]), dict(rules=z[84:100]),
                 dict(seg=z[100:108]), dict(cert=z[178:186]), dict(parts=z[194:206]), dict(refs=z[210:214]),
                 dict(old=z[232:264]), dict(summary=z[260:356]), dict(n=0xFFFFFFFF)]
        for change in cases:
            a = dict(good, **change)
            with pytest.raises(ramcrc.RamcrcError) as e:
                ramcrc._check(ramcrc.lib().ramcrc_replay_table_remove_device(
                    t._h, p(a["keys"]), 16, p(a["reqs"]), a["n"], p(a["hashes"]), p(a["rules"]), a["nv"], 0,
                    p(a["seg"]), p(a["out"]), a["cap"], p(a["cert"]), p(a["parts"]), p(a["refs"]), p(a["old"]),
                    p(a["summary"]), None), "remove")
            assert e.value.code == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
    finally:
        t.close()
