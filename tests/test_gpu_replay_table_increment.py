"""ramcrc_replay_table_increment_device: a multi-increment against the replay
table on the GPU (k_rm_group, k_inc_size, k_wr_scan, k_inc_emit), the loop of
MasterService::multiIncrement (src/MasterService.cc:1277-1330) over
incrementObject (:678-790).

The scenarios are increment_cases.py's, the ones
test_replay_table_increment_host.py runs on the host: every batch is walked by
ctx.segment_walk, the expectation (plain Python, held against the goldens and
the live query's winners) is what every device increment is held against, a
host table fed the same batches must give the same bytes, every call a write
can express is also held against ramcrc_replay_table_write_device, and the
output, walked with the call's certificate by ramcrc_replay_verify_device, is
added as the next batch.  Every output is pre-filled with 0xA5 and checked past
its end."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import increment_cases as ic
import lookup_cases as lc
import replay_table_cases as tc
import resolve_cases as rc
import write_cases as wc
from test_gpu_replay_table_lookup import grid_case  # noqa: F401  (the 249,165-record table)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = ic.FILL


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return ic.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_goldens(drv, oracle_mod):
    ref = ic.golden()
    assert ic.check_expectation_against_golden(oracle_mod, ref) == ref["steps"]
    ic.case_goldens(drv)


def test_closing_the_loop(drv):
    ic.case_closing_the_loop(drv)


def test_the_sum(drv):
    ic.case_sum(drv)


def test_reject_rules(drv):
    ic.case_reject_rules(drv)


def test_invalid_object(drv):
    ic.case_invalid_object(drv)


def test_duplicates(drv):
    ic.case_duplicates(drv)


def test_key_lengths(drv):
    ic.case_key_lengths(drv)


def test_value_alignment(drv):
    ic.case_value_alignment(drv)


def test_alignment(drv):
    ic.case_alignment(drv)


def test_space(drv):
    ic.case_space(drv)


def test_counts(drv):
    ic.case_counts(drv)


def test_bad_requests_and_bad_rules_among_good_ones(drv):
    ic.case_bad_requests(drv)


def test_nullable_arguments(drv):
    ic.case_nullable(drv)


def test_read_only(drv, mixed):
    ic.case_read_only(drv, mixed)


# --------------------------------------------------------------- grid size
def test_the_large_table_and_small_grids(ramcrc, oracle_mod, grid_case):  # noqa: F811
    """250,000 requests against the 249,165-record table at 1 and 3 CUs
    between two default-grid calls: every second one a present key, the others
    absent, every 97th a repeat of the request before it, and the capacity
    cuts the output inside its last tenth.

    The table's values have 64 bytes, so a device write first puts 8-byte
    values over three fifths of the present keys; walked and added, that is
    batch 2 (increment_cases.Large).  The parts, the references and the
    summary are held against numpy, the bytes against the host twin and the
    device's own walk and checksum pass, and the requests without the invalid
    objects against the write of their images."""
    ws, key_cap, kb, q, want = grid_case
    L = ic.Large(q, want, kb)
    nq, cap = L.nq, ws[0].cap
    seg_ids = np.array([500, 900, 1300], np.uint64)
    c = ramcrc.Context(0)
    tab = None
    try:
        drv = ic.DeviceDriver(ramcrc, oracle_mod, c)
        tab = ic.DeviceTab(drv, key_cap, 3)
        for w in ws:
            tab.add(w)
        # the 8-byte values: one write over the sample's keys
        data, wreqs = L.write_requests()
        ns = L.first.shape[0]
        nv = 1 << 33
        assert ns * 45 <= cap
        gw = wc.Written(c, tab.t, data, wreqs, cap, cap, nv, ic.TS, seg_ids=seg_ids[:2])
        assert gw.summary["ok"] == gw.summary["allocated"] == ns and gw.summary["out_bytes"] == 45 * ns
        buf = np.zeros(cap, np.uint8)
        buf[:45 * ns] = np.frombuffer(gw.out, np.uint8)
        assert tab.add(ac.Walked(c, buf, np.array([gw.cert], np.uint32), cap, 1, min_entry=40)) == 2
        nv += ns + 5
        L.expect(gw.parts["version"], nv)
        assert nq * 9 // 10 < L.first_out < nq and L.first_out % 256 not in (0, 255)   # the cut falls inside a tile
        n_ent = L.n_ok + L.n_tomb
        looked = lc.Looked(c, tab.t, kb, L.reqs).results
        base = None
        for ncu in (0, 1, 3, 0):
            c.set_cus(ncu)   # 0: every CU again
            g = ic.Incremented(c, tab.t, kb, L.reqs, L.args, L.cap, L.cap, nv, ic.TS, seg_ids=seg_ids)
            ic._check_got(g, nq, L.cap)
            L.held(g, looked, ("grid", ncu))
            if base is None:
                base = g
                # once: the host twin's bytes, and the device's own walk and checksum pass
                h = tab.host.increment_raw(kb, L.reqs, L.args, L.cap, nv, ic.TS, seg_ids=seg_ids, room=L.cap)
                ic.same_outputs(h, g)
                cap16 = -(-L.cap // 16) * 16
                d = torch.zeros(cap16, dtype=torch.uint8, device="cuda")
                d[:L.head] = g.d_out[:L.head]
                dc = torch.from_numpy(np.array([g.cert], np.uint32).view(np.int32)).cuda()
                st = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
                ent = torch.zeros((n_ent + 8, 4), dtype=torch.int32, device="cuda")
                dn = torch.zeros(1, dtype=torch.int64, device="cuda")
                crc = torch.zeros(n_ent + 8, dtype=torch.int32, device="cuda")
                c.replay_verify(d, cap16, cap16, 1, dc, st, ent, dn, crc)
                c.check()
                st = st.cpu().numpy().view(np.uint32)[0]
                assert int(st[0]) == segments.SEG_OK and int(st[2]) == n_ent == int(dn.item())
                assert int(st[3]) == 0
            else:
                assert g.out == base.out and g.cert == base.cert, ("grid", ncu)
        # the write of the images of the new values, without the invalid objects
        g = ic.Incremented(c, tab.t, kb, L.reqs[L.keep], L.args[L.keep], L.cap, L.cap, nv, ic.TS, seg_ids=seg_ids)
        data, wreqs = L.images(L.keep, L.bits[L.keep])
        L.held_to_the_write(g, wc.Written(c, tab.t, data, wreqs, L.cap, L.cap, nv, ic.TS, seg_ids=seg_ids))
    finally:
        if tab is not None:
            tab.close()
        c.close()


# ----------------------------------------------------------- spoiled tables
def test_a_spoiled_table(ramcrc, oracle_mod):
    """Spoiled by the key capacity: every pre-filled output but the summary
    stays untouched, the summary is zero with spoiled = 1, the increment raises
    no refusal of its own, and after the reset the table takes increments
    again."""
    c = ramcrc.Context(0)
    drv = ic.DeviceDriver(ramcrc, oracle_mod, c)
    keys = [(7, b"cap key 3"), (1, b"fresh")]
    kb, reqs = segments.lookup_queries(keys)
    args = segments.increment_args([ic.ARG] * 2)
    try:
        full = drv.batch([[tc.head(1)] + [rc.obj(7, b"cap key %d" % k, 2, ic.i64(k)) for k in range(64)]])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        tab = drv.table(64, 4)
        try:
            tab.add(full)
            g, w = ic.increment(tab, ic.checked(tab), keys, args, what="before")
            assert w.summary["ok"] == 2 and w.summary["created"] == 1
            tc.Added(more).add(tab.t)
            with pytest.raises(ramcrc.RamcrcError) as e:
                c.check()
            assert e.value.code == ramcrc.EREFUSED
            for kw in (dict(), dict(want_refs=False, want_old=False)):
                g = ic.Incremented(c, tab.t, kb, reqs, args, 4096, 4096, **kw)   # its check() passes: nothing is refused anew
                assert g.summary == ic.SPOILED_SUMMARY and (g.summary_past == FILL).all()
                for a in (g.out_all, g.parts, g.parts_past, g.cert_past, g.refs, g.old):
                    assert a is None or (np.ascontiguousarray(a).view(np.uint8) == FILL).all()
                assert g.cert == (ic.FILL32, ic.FILL32)
            tab.reset()
            tab.add(full)
            ic.increment(tab, ic.checked(tab), keys, args, what="after the reset")
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
                    cap=64, cert=z[176:184], parts=z[192:212], refs=z[224:232], old=z[256:288], summary=z[320:464],
                    args=z[480:496], n=1)
        assert all(p(v) % 16 == 0 for k, v in good.items() if k not in ("nv", "cap", "n"))
        cases = [dict(nv=0), dict(summary=None), dict(cert=None), dict(reqs=None), dict(args=None), dict(parts=None),
                 dict(out=None), dict(keys=None), dict(reqs=z[36:60]), dict(args=z[484:500]), dict(hashes=z[68:76]),
                 dict(rules=z[84:100]), dict(seg=z[100:108]), dict(cert=z[178:186]), dict(parts=z[194:214]),
                 dict(refs=z[228:236]), dict(old=z[264:296]), dict(summary=z[324:468]), dict(n=0xFFFFFFFF)]
        for change in cases:
            a = dict(good, **change)
            with pytest.raises(ramcrc.RamcrcError) as e:
                ramcrc._check(ramcrc.lib().ramcrc_replay_table_increment_device(
                    t._h, p(a["keys"]), 16, p(a["reqs"]), a["n"], p(a["args"]), p(a["hashes"]), p(a["rules"]),
                    a["nv"], 0, p(a["seg"]), p(a["out"]), a["cap"], p(a["cert"]), p(a["parts"]), p(a["refs"]),
                    p(a["old"]), p(a["summary"]), None), "increment")
            assert e.value.code == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
    finally:
        t.close()
