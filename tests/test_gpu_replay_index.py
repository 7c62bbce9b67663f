"""ramcrc_replay_table_index_build_device and ramcrc_index_lookup_device: the
secondary index built and searched on the GPU (k_ix_size, k_ix_scan, k_ix_emit,
k_ix_sort, k_ix_merge, k_ix_hashes; k_ixl_search, k_ixl_scan, k_ixl_copy, k_ixl_long),
IndexletManager::lookupIndexKeys (src/IndexletManager.cc:611-709) over entries
sorted as key_less sorts them.

The scenarios are index_cases.py's, the ones test_replay_index_host.py runs on
the host: every batch is walked by ctx.segment_walk, the expectation (plain
Python, held against the goldens and the live query's winners) is what every
device call is held against, and a host table fed the same batches must give
the same entries (key_off dereferenced), the same hashes and the same lookup
replies, byte for byte.  Every output is pre-filled with 0xA5 and checked past
its end."""
import numpy as np
import pytest

from ramcloud_amd import segments

import index_cases as ix
import lookup_cases as lc
import replay_table_cases as tc
import resolve_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = ix.FILL
T = ix.source_constants()["kIxTile"]


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drv(ramcrc, oracle_mod, ctx):
    return ix.DeviceDriver(ramcrc, oracle_mod, ctx)


@pytest.fixture(scope="module")
def mixed(drv):
    return lc.mixed_batches(drv)


def test_goldens(drv):
    ix.case_goldens(drv)


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T, 5 * T + 3])
def test_sort_edges_ascending_descending_equal(drv, n):
    """Entry counts around the LDS tile and odd run counts in every merge
    pass; the entries arrive (in slot order) ascending, descending and all
    equal in key."""
    ix.case_sort(drv, n)


def test_sort_with_room_to_spare(drv):
    """entry_capacity asks for more merge passes than the entries need: the
    spare passes copy."""
    ix.case_sort(drv, T + 1, extra=2 * T)


def test_comparator(drv):
    ix.case_comparator(drv)


def test_selection(drv):
    ix.case_selection(drv)


def test_capacity(drv):
    ix.case_capacity(drv)


def test_lookup(drv):
    ix.case_lookup(drv)


def test_long_runs(drv):
    ix.case_long_runs(drv)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_chain_build_lookup_read_hashes(drv, seed):
    ix.case_chain(drv, seed)


def test_read_only(drv, mixed):
    """The build leaves lookups, live lists, stats and every batch array unchanged."""
    ix.case_read_only(drv, mixed)


def test_build_lookup_and_read_hashes_chain_on_one_stream(drv, ctx):
    """No sync between the three calls: the lookup reads n_entries from the
    build's summary on the device, and read_hashes takes the lookup's hashes
    where they lie."""
    objs = ix.lookup_table(drv)
    tab = ix.hashed_table(drv, 64, objs)
    try:
        fill = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
        d_e, d_h, d_k, d_bs = fill(32 * 64), fill(8 * 64).view(torch.int64), fill(1024), fill(56).view(torch.int64)
        kb, q = segments.index_queries([(b"run", b"run", 0, 100)])
        d_qk = torch.from_numpy(kb).cuda()
        d_q = torch.from_numpy(q.view(np.uint8).copy()).cuda().view(torch.int64)
        d_out, d_res, d_ls = fill(8 * 4).view(torch.int64), fill(48).view(torch.int64), fill(48).view(torch.int64)
        d_reply, d_rs = fill(4096), fill(72).view(torch.int64)
        idx = tab.t.index_build(1, 1, d_e, d_h, d_k, d_bs)
        ctx.index_lookup(idx, d_qk, d_q, d_out, d_res, d_ls)
        tab.t.read_hashes(1, d_out, d_reply, d_rs, 1 << 40, n_hashes=4)
        ctx.check()
        assert d_out.cpu().numpy().view(np.uint64).tolist() == [10, 20, 30, 40]
        rs = d_rs.cpu().numpy().view(segments.READ_HASHES_SUMMARY_DTYPE)[0]
        assert int(rs["hashes"]) == 4 and int(rs["objects"]) == 4
    finally:
        tab.close()


# --------------------------------------------------------------- grid size
@pytest.mark.parametrize("ncu", [1, 2, 3])
def test_small_grids(ramcrc, oracle_mod, ncu):
    """Grids sized for 1, 2 and 3 CUs (8 workgroups of 256 lanes a CU): 2T + 1
    entries a table id in a table of 8,192 slots take a 1-CU grid several
    tiles a workgroup in the slot passes; more queries than two tiles."""
    c = ramcrc.Context(0)
    try:
        c.set_cus(ncu)
        d = ix.DeviceDriver(ramcrc, oracle_mod, c)
        ix.case_sort(d, 2 * T + 1)
        ix.case_lookup(d)
        ix.case_long_runs(d)
    finally:
        c.close()


# ----------------------------------------------------------- spoiled tables
def test_spoiled_tables(ramcrc, oracle_mod):
    """Spoiled by the key capacity: the pre-filled arrays stay untouched, the
    summary is zero with spoiled = 1, the call raises no refusal of its own, a
    lookup against that build serves nothing, and after the reset the table
    builds again."""
    c = ramcrc.Context(0)
    drv = ix.DeviceDriver(ramcrc, oracle_mod, c)
    try:
        full = drv.batch([tc.capacity_lists(64)])
        more = drv.batch([[tc.head(2), rc.obj(7, b"one more key", 1)]])
        tab = drv.table(64, 4)
        try:
            tab.add(full)
            tc.Added(more).add(tab.t)
            with pytest.raises(ramcrc.RamcrcError) as e:
                c.check()
            assert e.value.code == ramcrc.EREFUSED
            g = ix.DevBuilt(c, tab.t, 7, 1, 8, 64)   # check() passes
            assert g.summary == dict(ix.ZERO_BSUM, spoiled=1) and g.entries == []
            ix.lookup(drv, g, [], [(b"", b"", 0, 4), (b"a", b"b", 0, 1)], what="a spoiled build", dead=True)
            tab.reset()
            tab.add(full)
            ix.build(tab, ix.WantIndex([], 64), 7, 1, what="after the reset")
        finally:
            tab.close()
    finally:
        c.close()


def test_bad_arguments(ctx, ramcrc):
    """index_id 0, missing or misaligned arrays, capacities past 2^32 are
    EINVAL before any launch: nothing is written and the context stays
    clean."""
    t = ramcrc.ReplayTable(ctx, 64, 1)
    try:
        z = torch.full((2048,), FILL, dtype=torch.uint8, device="cuda")
        p = lambda x: None if x is None else x.data_ptr()
        good = dict(iid=1, entries=z[0:256], ecap=8, hashes=z[256:320], keys=z[512:576], kcap=64, summary=z[1024:1080])
        assert p(good["entries"]) % 16 == 0 and p(good["summary"]) % 8 == 0
        L = ramcrc.lib().ramcrc_replay_table_index_build_device
        call = lambda a, h=t._h: L(h, 1, a["iid"], p(a["entries"]), a["ecap"], p(a["hashes"]), p(a["keys"]), a["kcap"],
                                   p(a["summary"]), None)
        cases = [dict(iid=0), dict(entries=None), dict(hashes=None), dict(keys=None), dict(summary=None),
                 dict(entries=z[8:264]), dict(hashes=z[260:324]), dict(summary=z[1028:1084]), dict(ecap=(1 << 32) - 1)]
        for change in cases:
            assert call(dict(good, **change)) == ramcrc.EINVAL, change
        assert call(good, None) == ramcrc.EINVAL
        LL = ramcrc.lib().ramcrc_index_lookup_device
        lgood = dict(ctx=ctx._h, entries=z[0:256], hashes=z[256:320], keys=z[512:576], bsum=z[1024:1080], qkeys=z[1100:1110],
                     qbytes=10, q=z[1200:1240], nq=1, out=z[1280:1312], ocap=4, res=z[1400:1448], summary=z[1600:1648])
        lcall = lambda a: LL(a["ctx"], p(a["entries"]), p(a["hashes"]), p(a["keys"]), p(a["bsum"]), p(a["qkeys"]),
                             a["qbytes"], p(a["q"]), a["nq"], p(a["out"]), a["ocap"], p(a["res"]), p(a["summary"]), None)
        for change in (dict(ctx=None), dict(bsum=None), dict(summary=None), dict(q=None), dict(res=None), dict(qkeys=None),
                       dict(out=None), dict(nq=(1 << 32) - 1), dict(q=z[1204:1244]), dict(out=z[1284:1316]),
                       dict(res=z[1404:1452]), dict(summary=z[1604:1652]), dict(bsum=z[1028:1084]),
                       dict(entries=z[8:264]), dict(hashes=z[260:324])):
            assert lcall(dict(lgood, **change)) == ramcrc.EINVAL, change
        ctx.check()
        assert (z.cpu().numpy() == FILL).all()
        for change in (dict(), dict(entries=None, hashes=None, ecap=0), dict(keys=None, kcap=0), dict(iid=255), dict(iid=70000)):
            assert call(dict(good, **change)) == 0, change
        ctx.check()
        s = z[1024:1080].cpu().numpy().view(ix.BSUM)[0]
        assert ix.sdict(s, ix.BSUM.names) == ix.ZERO_BSUM and (z[0:1024].cpu().numpy() == FILL).all()
    finally:
        t.close()


def test_the_calls_do_not_allocate_after_reserve(ramcrc, oracle_mod):
    """After ramcrc_ctx_reserve(ctx, 32 + 16 * ceil(S / 256), 4 * entry_capacity)
    a build takes no scratch, and after reserve(32 + 16 * ceil(n / 256), 2 * n)
    a lookup of n queries takes none, as the header states."""
    c2 = ramcrc.Context(0)   # a context that has reserved nothing yet
    drv = ix.DeviceDriver(ramcrc, oracle_mod, c2)
    tab = None
    try:
        n = T + 5
        objs = [(1, b"k %06d" % (7919 * i % n), i) for i in range(n)]
        tab = ix.hashed_table(drv, 3000, objs)
        S = ix.cl.rc_slots(3000)
        pairs = [(k, h) for _, k, h in objs]
        nq = 300
        ranges = [(b"k %06d" % i, b"k %06d" % (i + 2), 0, 10) for i in range(nq)]
        c2.reserve(max(32 + 16 * -(-S // 256), 32 + 16 * -(-nq // 256)), max(4 * (n + 3), 2 * nq))
        before = ramcrc.scratch_allocations()
        g = ix.DevBuilt(c2, tab.t, 1, 1, n + 3, 9 * n)
        kb, q = segments.index_queries(ranges)
        r = ix.DevReply(c2, g, kb, q, 3 * nq)
        assert ramcrc.scratch_allocations() == before
        w = ix.WantIndex(pairs, n)
        assert g.entries == w.entries and g.hashes == w.hashes
        want, sm = ix.expect_lookup(w.pairs, ranges)
        assert r.reply == want and r.summary == sm
    finally:
        if tab is not None:
            tab.close()
        c2.close()
