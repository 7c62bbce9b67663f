"""ramcrc_replay_table_clean_device and ramcrc_replay_table_clean_size_device:
cleaning batches out of the replay table on the GPU (k_clean_open,
k_clean_mark, k_clean_scan, k_clean_move, k_clean_claims), the relocation step
of the log cleaner (LogCleaner::relocateLiveEntries, src/LogCleaner.cc:575-722,
over ObjectManager::relocateObject and relocateTombstone).

The scenarios are clean_cases.py's, the ones test_replay_table_clean_host.py
runs on the host: every device clean is held against the plain-Python
expectation and against a host table fed the same batches, byte for byte; the
survivor is walked by ctx.segment_walk under the call's certificate; every
output is pre-filled with 0xA5 and checked past its end; after the call every
victim array is overwritten with 0xA5 before the table is asked again."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import clean_cases as cc
import lookup_cases as lc
import remove_cases as rm
import replay_table_cases as tc
import resolve_cases as rc
from test_gpu_replay_table_lookup import grid_case  # noqa: F401  (the 249,165-record table)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = cc.FILL


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return cc.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


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


# --------------------------------------------------------------- grid size
class Copy:
    """A walked batch on tensors of its own, so that they can be overwritten."""

    def __init__(self, w):
        self.d, self.d_status, self.d_entries, self.d_n = (x.clone() for x in (w.d, w.d_status, w.d_entries, w.d_n))
        self.cap, self.nseg, self.table, self.status, self.buf = w.cap, w.nseg, w.table, w.status, w.buf


def test_small_grids_and_no_allocation(ramcrc, oracle_mod, grid_case):  # noqa: F811
    """The 249,165-record table with about half its records dead: batch 1
    repeats a segment of batch 0 (equal versions: the lower batch keeps the
    keys) and batch 2 holds the tombstones of 42,000 objects of batch 0.
    Batches 0 and 1 are cleaned at 1 and 3 CUs between two default-grid calls,
    on a fresh table each time; every call must write the first one's bytes.

    The victims' record tables hold 262,146 and 131,073 slots: 1,025 and 513
    tiles of 256.  The grids are capped at 8 workgroups per CU: at 1 CU 8
    workgroups take the 1,538 tiles in 193 passes, at 3 CUs 24 in 65; the
    scan's one workgroup takes them in 7 steps of 256.

    Every round has a context of its own, which before the clean has served
    only the adds, one remove of 42,000 keys, a walk and a lookup: its scratch
    is below what the header states for the clean, so the stated reserve has to
    allocate, and behind it clean_size and clean must not: the library's count
    of scratch allocations stays.  At the end (P4) one more batch overwrites
    two moved keys and is resolved through the re-pointed slots."""
    ws, key_cap, kb, q, want = grid_case
    hits = np.flatnonzero(want["kind"] == lc.OBJECT)[:42000]
    reqs = q[hits].copy()
    rcap = 42 * hits.size + 6
    rcap16 = -(-rcap // 16) * 16
    first = None
    for ncu in (0, 1, 3, 0):
        c = ramcrc.Context(0)
        tabs = []
        try:
            t = ramcrc.ReplayTable(c, key_cap, 5)
            tabs.append(t)
            added = [tc.Added(Copy(w)) for w in ws]
            for a in added:
                a.add(t)
            r = rm.Removed(c, t, kb, reqs, rcap, rcap, 1 << 33)
            assert r.summary["removed"] == hits.size
            buf = np.zeros(rcap16, np.uint8)
            buf[:len(r.out)] = np.frombuffer(r.out, np.uint8)
            w2 = ac.Walked(c, buf, np.array([r.cert], np.uint32), rcap16, 1, min_entry=42)
            a2 = tc.Added(w2)
            assert a2.add(t) == 2
            before = lc.Looked(c, t, kb, q).results.copy()
            assert (before["kind"][hits] == lc.TOMBSTONE).all() and (before["batch"][hits] == 2).all()
            # sizes from clean_size, after the reserve the header states
            d_sum = torch.zeros(14, dtype=torch.int64, device="cuda")
            d_usage = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
            allocs = ramcrc.scratch_allocations()
            c.reserve(ramcrc.ReplayTable.clean_reserve([a.w.d_entries.shape[0] for a in added]), 0)
            assert ramcrc.scratch_allocations() > allocs, "the context already had the clean's scratch"
            allocs = ramcrc.scratch_allocations()
            t.clean_size([0, 1], d_sum, usage=d_usage)
            c.check()
            assert ramcrc.scratch_allocations() == allocs, "clean_size allocated after the stated reserve"
            sm = cc.summary_dict(d_sum.cpu().numpy().view(cc.SUMMARY)[0])
            n0, n1 = ws[0].table.shape[0], ws[1].table.shape[0]
            assert sm["records"] == n0 + n1 and sm["needed_records"] == n0 - hits.size
            assert sm["dropped_objects"] == n1 + hits.size and sm["dropped_other"] == 0
            cap = -(-sm["needed_bytes"] // 16) * 16
            ecap = sm["needed_records"]
            c.set_cus(ncu)   # 0: every CU again
            g = cc.Cleaned.__new__(cc.Cleaned)
            fill = lambda n, dt: torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt)
            outs = dict(out=fill(cap + cc.PAD, torch.uint8), cert=fill(8 + cc.PAD, torch.int32),
                        status=fill(16 + cc.PAD, torch.int32), entries=fill(16 * ecap + cc.PAD, torch.int32).view(-1, 4),
                        n=fill(8 + cc.PAD, torch.int64), work=fill(8 * ecap + cc.PAD, torch.int64),
                        moved=fill(8 * ecap + cc.PAD, torch.int32).view(-1, 2),
                        usage=fill(64 + cc.PAD, torch.int64), summary=fill(112 + cc.PAD, torch.int64))
            batch = t.clean([0, 1], outs["out"], outs["cert"], outs["status"], outs["entries"][:ecap], outs["n"],
                            outs["work"], outs["summary"], moved=outs["moved"], usage=outs["usage"],
                            out_capacity=cap)
            c.check()
            assert ramcrc.scratch_allocations() == allocs, "clean allocated after the stated reserve"
            c.set_cus(0)
            assert batch == 3
            g.nvic, g.cap, g.ecap = 2, cap, ecap
            g.d_out, g.d_cert, g.d_status, g.d_entries, g.d_n = (outs[k] for k in ("out", "cert", "status", "entries", "n"))
            g.d_work, g.d_moved, g.d_usage, g.d_sum = (outs[k] for k in ("work", "moved", "usage", "summary"))
            g.read()
            assert g.summary == dict(sm, batch=3), ("grid", ncu, g.summary)
            assert lc.same(g.usage, d_usage.cpu().numpy().view(np.uint8).reshape(-1)[:64].view(cc.USAGE))
            # P1: the same answers, victim references mapped through d_moved
            new = np.full(n0, -1, np.int64)
            assert (g.moved["batch"] == 0).all()
            new[g.moved["record"]] = np.arange(ecap)
            want_after = before.copy()
            in0 = before["batch"] == 0
            assert (new[before["record"][in0]] >= 0).all()
            want_after["record"][in0] = new[before["record"][in0]]
            want_after["batch"][in0] = 3
            want_after["segment"][in0] = 0
            rows = g.table[want_after["record"][in0].astype(np.int64)]
            want_after["value_off"][in0] = rows[:, 1] + 2 + 35
            # P4: the victims' arrays are 0xA5 from here on
            for a in added:
                for x in (a.w.d, a.w.d_status, a.w.d_entries, a.w.d_n, a.d_work):
                    x.view(torch.uint8).fill_(FILL)
            after = lc.Looked(c, t, kb, q).results
            assert lc.same(after, want_after), ("grid", ncu, "answers after the clean")
            # P3: the device's own walk and checksum pass over the survivor
            d = g.d_out[:cap]
            st = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
            ent = torch.zeros((ecap + 8, 4), dtype=torch.int32, device="cuda")
            dn = torch.zeros(1, dtype=torch.int64, device="cuda")
            crc = torch.zeros(ecap + 8, dtype=torch.int32, device="cuda")
            c.replay_verify(d, cap, cap, 1, g.d_cert[:2], st, ent, dn, crc)
            c.check()
            st = st.cpu().numpy().view(np.uint32)
            assert int(dn.item()) == g.n == ecap and int(st[0, 3]) == 0
            assert lc.same(st[0, :3], g.status[0, :3]) and int(st[0, 0]) == segments.SEG_OK
            assert lc.same(ent[:ecap].cpu().numpy().view(np.uint32), g.table), "the walk's record table"
            if first is None:
                first = g
                # once: the host twin's bytes
                twin = ramcrc.ReplayTableHost(key_cap, 4)
                try:
                    for w in list(ws) + [w2]:
                        twin.add(w.buf, w.cap, w.nseg, w.status, w.table)
                    h = twin.clean([0, 1], cap, ecap, fill=FILL)
                    assert cc.summary_dict(h["summary"]) == g.summary
                    assert h["out"][:g.summary["out_bytes"]].tobytes() == g.out
                    assert tuple(int(x) for x in h["cert"]) == g.cert
                    assert lc.same(h["entries"], g.table) and lc.same(h["moved"], g.moved)
                    assert lc.same(h["usage"], g.usage)
                    h_res, _ = twin.lookup(kb, q)
                    assert lc.same(h_res, after)
                finally:
                    twin.close()
            else:
                assert g.out == first.out and g.cert == first.cert, ("grid", ncu)
                assert lc.same(g.table, first.table) and lc.same(g.moved, first.moved), ("grid", ncu)
            # P4's last step: one more batch over two moved keys, an object above
            # the first and a tombstone of the second's version
            i0, i1 = (int(x) for x in np.flatnonzero(in0)[:2])
            key_of = lambda i: (int(q["table_id"][i]), kb[int(q["key_off"][i]):int(q["key_off"][i]) + 8].tobytes())
            v0, v1 = int(before["version"][i0]), int(before["version"][i1])
            es = [rc.obj(*key_of(i0), v0 + 1, b"after the clean"), rc.tomb(*key_of(i1), v1)]
            sbuf, scerts = ac.source_of(oracle_mod, [es], 4096)
            assert tc.Added(ac.Walked(c, sbuf, scerts, 4096, 1)).add(t) == 4
            pick = np.array([i0, i1])
            more = lc.Looked(c, t, kb, q[pick]).results
            assert more["batch"].tolist() == [4, 4] and more["record"].tolist() == [0, 1], ("grid", ncu)
            assert more["version"].tolist() == [v0 + 1, v1], ("grid", ncu)
            assert more["kind"].tolist() == [lc.OBJECT, lc.TOMBSTONE], ("grid", ncu)
            rest = np.setdiff1d(np.arange(q.shape[0])[::997], pick)
            assert lc.same(lc.Looked(c, t, kb, q[rest]).results, want_after[rest]), ("grid", ncu)
        finally:
            for t in tabs:
                t.close()
            c.close()


def test_bad_arguments(ctx, ramcrc):
    """Rule 10: missing and misaligned arrays, a capacity that is no multiple
    of 16 and a record capacity of 2^32 are EINVAL before any launch: nothing
    is written, no number is taken and the context stays clean."""
    t = ramcrc.ReplayTable(ctx, 64, 4)
    try:
        w = ac.Walked(ctx, np.zeros(64, np.uint8), np.array([[0, 0]], np.uint32), 64, 1)
        tc.Added(w).add(t)
        z = torch.full((1024,), FILL, dtype=torch.uint8, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()
        vic = np.array([0], np.uint32)
        good = dict(t=t._h, vic=vic.ctypes.data, n=1, out=z[0:64], cap=64, cert=z[64:72], status=z[80:96],
                    entries=z[96:160], ecap=4, n_entries=z[160:168], work=z[176:208], moved=z[208:240],
                    usage=z[240:272], summary=z[288:400])
        cases = [dict(t=None), dict(vic=None), dict(n=0), dict(summary=None), dict(cert=None), dict(status=None),
                 dict(n_entries=None), dict(entries=None), dict(work=None), dict(out=None), dict(cap=72),
                 dict(ecap=1 << 32), dict(out=z[8:72]), dict(cert=z[66:74]), dict(status=z[82:98]),
                 dict(entries=z[104:168]), dict(n_entries=z[164:172]), dict(work=z[180:212]),
                 dict(moved=z[212:244]), dict(usage=z[244:276]), dict(summary=z[292:404])]
        L = ramcrc.lib()
        ptr = lambda v: p(v) if hasattr(v, "data_ptr") else v   # (the handle and the host list go as they are)
        for change in cases:
            a = {k: ptr(v) if k not in ("n", "cap", "ecap") else v for k, v in dict(good, **change).items()}
            rcode = L.ramcrc_replay_table_clean_device(
                a["t"], a["vic"], a["n"], a["out"], a["cap"], a["cert"], a["status"], a["entries"], a["ecap"],
                a["n_entries"], a["work"], a["moved"], a["usage"], a["summary"], None, None)
            assert rcode == ramcrc.EINVAL, change
        for change in (dict(t=None), dict(vic=None), dict(n=0), dict(summary=None), dict(usage=z[244:276]),
                       dict(summary=z[292:404])):
            a = {k: ptr(v) if k not in ("n", "cap", "ecap") else v for k, v in dict(good, **change).items()}
            rcode = L.ramcrc_replay_table_clean_size_device(a["t"], a["vic"], a["n"], a["usage"], a["summary"], None)
            assert rcode == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
        s = tc.device_stats(ctx, t)
        assert s["batches"] == 1 and s["spoiled"] == 0
    finally:
        t.close()
