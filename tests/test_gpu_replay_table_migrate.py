"""ramcrc_replay_table_migrate_device: a tablet migration's source side on the
GPU (k_mig_size, k_mig_cut, k_mig_emit, k_mig_seal), MasterService::
migrateTablet (src/MasterService.cc:1084-1225) over migrateSingleLogEntry
(:935-1073) against the replay table.

The scenarios are migrate_cases.py's, the ones
test_replay_table_migrate_host.py runs on the host: every device call is held
against the plain-Python expectation and against a host table fed the same
batches, byte for byte; every output is pre-filled with 0xA5 and checked at and
past every head and past segments_used; the chain walks the transfer segments
on the device under the call's certificates and adds them to a second table."""
import numpy as np
import pytest

from ramcloud_amd import segments

import lookup_cases as lc
import migrate_cases as mg
import partition_cases as pc
import replay_table_cases as tc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return mg.DeviceDriver(ramcrc, oracle_mod, ctx)


def test_reference_fixture(drv):
    mg.check_fixture(drv, pc.load("migrate_ref.json"))


def test_counts(drv):
    mg.case_counts(drv)


def test_boundaries(drv):
    mg.case_boundaries(drv)


def test_entry_sizes(drv):
    mg.case_entry_sizes(drv)


def test_hash_range(drv):
    mg.case_hash_range(drv)


def test_liveness(drv):
    mg.case_liveness(drv)


def test_foreign_records(drv):
    mg.case_foreign(drv)


def test_cursor(drv):
    mg.case_cursor(drv)


def test_arguments(drv):
    mg.case_arguments(drv)


def test_spoiled(drv):
    mg.case_spoiled(drv)


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_chain(drv, seed):
    mg.case_chain(drv, seed)


def test_bad_device_arguments(drv, ramcrc, ctx):
    """Rule 7's pointer rules: missing and misaligned arrays are EINVAL before
    any launch, and nothing is written."""
    tab = drv.tab(64, 2)
    try:
        tab.add([[mg.head(), mg.rc.obj(7, b"k", 1, b"v")]], 4 * 1024)
        z = torch.full((1024,), mg.FILL, dtype=torch.uint8, device="cuda")
        lst = np.array([0], np.uint32)
        good = dict(t=tab.t._h, lst=lst.ctypes.data, n=1, out=z[0:128], certs=z[128:144], counts=z[144:176],
                    sent=z[176:240], sent_cap=8, first=z[240:256], summary=z[256:376])
        cases = [dict(t=None), dict(lst=None), dict(n=0), dict(summary=None), dict(certs=None), dict(counts=None),
                 dict(out=None), dict(out=z[8:136]), dict(certs=z[130:146]), dict(counts=z[146:178]),
                 dict(sent=z[180:244]), dict(sent=None), dict(first=z[244:260]), dict(summary=z[260:380])]
        p = lambda v: v.data_ptr() if hasattr(v, "data_ptr") else v
        for change in cases:
            a = {k: p(v) for k, v in dict(good, **change).items()}
            rcode = ramcrc.lib().ramcrc_replay_table_migrate_device(
                a["t"], a["lst"], a["n"], 7, 0, mg.M64, 0, 0, 0, a["out"], 64, 64, 2, a["certs"], a["counts"],
                a["sent"], a["sent_cap"], a["first"], a["summary"], None)
            assert rcode == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == mg.FILL).all()
    finally:
        tab.close()


def test_small_grids_and_no_allocation(ramcrc, oracle_mod):
    """migrate_cases.count_lists (1,549 records of one segment in a record
    table of 65,537 slots: 257 tiles of 256) migrated at 1, 2 and 3 CUs between two
    default-grid calls: the grids are capped at 8 workgroups per CU, so at 1 CU
    8 workgroups take the tiles in 33 passes; every call must write the first
    one's bytes.  Every round has a context of its own that has served only the
    add: the stated reserve has to allocate, and behind it the call must not."""
    first = None
    for ncu in (0, 1, 2, 3, 0):
        c = ramcrc.Context(0)
        tab = mg.DeviceTab(mg.DeviceDriver(ramcrc, oracle_mod, c), 4096, 2)
        try:
            tab.add(mg.count_lists(), mg.COUNT_CAP)
            ecap = tab.added[0].w.d_entries.shape[0]
            assert ecap == 65537
            allocs = ramcrc.scratch_allocations()
            c.reserve(*ramcrc.ReplayTable.migrate_reserve([ecap], 80))
            assert ramcrc.scratch_allocations() > allocs, "the context already had the migration's scratch"
            allocs = ramcrc.scratch_allocations()
            c.set_cus(ncu)   # 0: every CU again
            got = []
            for t in (104, 101):
                for live in (False, True):
                    d = tab.launch([0], t, 512, 80, live_only=live)
                    c.check()
                    got.append(tab.read(d))
            assert ramcrc.scratch_allocations() == allocs, "migrate allocated after the stated reserve"
            c.set_cus(0)
            assert got[0].summary["sent_objects"] == 3 * mg.TILE + 5 and got[0].summary["segments_used"] > 60
            # every round against the expectation over its own walk's table, and
            # (the batch is one segment: its record order is the same in every
            # round) against the first round's bytes
            for g, (t, live) in zip(got, ((104, False), (104, True), (101, False), (101, True))):
                mg.check(g, tab.model.expect(oracle_mod, [0], t, 512, 80, live_only=live), ("grid", ncu, t, live))
            if first is None:
                first = got
            else:
                for g, f in zip(got, first):
                    mg.same_got(g, f, ("grid", ncu))
        finally:
            tab.close()
            c.close()


def test_migrate_walk_add_on_one_stream(drv, ctx, ramcrc):
    """The call, a walk of its outputs under its certificates and the add into
    a second table, on one stream without a sync or a check in between."""
    src = drv.tab(4096, 8)
    dst = ramcrc.ReplayTable(ctx, 4096, 2)
    try:
        for es in mg.chain_lists(34):
            src.add([es], 64 * 1024)
        lst, tid, cap = [0, 1, 2, 3], 1, 512
        want = src.model.expect(drv.oracle, lst, tid, cap, 64, live_only=True)   # (winners only: no ties at the destination)
        K = want.summary["segments_used"]
        assert K > 2 and want.summary["done"] == 1
        st = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
        ent = torch.zeros((K * (cap // 27 + 1), 4), dtype=torch.int32, device="cuda")
        dn = torch.zeros(1, dtype=torch.int64, device="cuda")
        work = torch.zeros(ent.shape[0], dtype=torch.int64, device="cuda")
        d = src.launch(lst, tid, cap, K, live_only=True)
        data = d["out"][:K * cap]
        assert dst.receive_migration(data, cap, cap, K, d["certs"][:2 * K].view(-1, 2), st, ent, dn, work) == 0
        ctx.check()
        mg.check(src.read(d), want, "chained on one stream")
        stn = st.cpu().numpy().view(np.uint32)
        assert (stn[:, 0] == segments.SEG_OK).all() and stn[:, 1].tolist() == [x[1] for x in want.certs]
        assert int(dn.item()) == want.summary["sent_objects"] + want.summary["sent_tombstones"]
        keys = [k for k in sorted(src.model.win) if k[0] == tid]
        kb, q = segments.lookup_queries(keys)
        a = lc.Looked(ctx, src.t, kb, q).results
        b = lc.Looked(ctx, dst, kb, q).results
        assert (a["kind"] == b["kind"]).all() and (a["version"] == b["version"]).all()
        assert (a["value_len"] == b["value_len"]).all() and (b["kind"] != lc.ABSENT).all()
    finally:
        src.close()
        dst.close()
