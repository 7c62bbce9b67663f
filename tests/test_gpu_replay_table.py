"""ramcrc_replay_table_*: ramcrc_replay_resolve_device's decision fed batch by
batch into a table that stays on the GPU (MasterService::recover replays
recovery segments as they arrive, src/MasterService.cc:3501-3720).

Every batch is walked by ctx.segment_walk on the device.  After the adds the
live query of every batch must equal the one-call resolve of the concatenation
of the batches (replay_table_cases.expect: ramcrc_replay_resolve_host, held
against the plain-Python replay) mapped back to {batch, record}, and the host
table's answer.  Every output is pre-filled with 0xA5, so a write past an end
shows.  test_replay_table_host.py runs the same cases on the host."""
import numpy as np
import pytest

from ramcloud_amd import segments

import append_cases as ac
import partition_cases as pc
import replay_table_cases as tc
import resolve_cases as rc
from append_cases import Walked, _u32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KiB = 1024
MiB = 1 << 20
FILL32 = tc.FILL32


@pytest.fixture(scope="module")
def ctx(ramcrc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = ramcrc.Context(0)
    yield c
    c.close()


def _walked(ctx, oracle, lists, cap=64 * KiB, bad=()):
    buf, certs = ac.source_of(oracle, lists, cap)
    for s in bad:
        certs[s, 1] ^= 1
    return Walked(ctx, buf, certs, cap, len(lists))


def _host_table(ramcrc, ws, key_cap, hashes=None):
    """The host form over the same batches: [(winner, live, counts)]."""
    t = ramcrc.ReplayTableHost(key_cap, len(ws))
    for j, w in enumerate(ws):
        t.add(w.buf, w.cap, w.nseg, w.status, w.table, key_hash=None if hashes is None else hashes[j])
    out = [t.live(j) for j in range(len(ws))]
    st = tc.stats_dict(t.stats())
    t.close()
    return out, st


def _same_as_host(ramcrc, ws, key_cap, lives, stats, hashes=None):
    host, h_stats = _host_table(ramcrc, ws, key_cap, hashes)
    for w, r, (h_winner, h_live, h_need, h_counts) in zip(ws, lives, host):
        n = w.table.shape[0]
        assert np.array_equal(r.winner_all[:n].reshape(-1).view(tc.REF), h_winner), "host and device winners"
        assert h_need == r.need and np.array_equal(h_live, r.live) and rc.counts_dict(h_counts) == r.counts
    assert stats == h_stats


@pytest.fixture(scope="module")
def relations(ctx, ramcrc, oracle_mod):
    """(walked batches, expectation after 1, 2 and 3 adds): computed once."""
    ws = [_walked(ctx, oracle_mod, [es]) for es in tc.relation_lists()]
    return ws, [tc.expect(ramcrc, ws[:k + 1]) for k in range(3)]


@pytest.fixture(scope="module")
def mixed(ctx, oracle_mod):
    return [_walked(ctx, oracle_mod, [es], rc.MIXED_CAP, bad=[0] if j == rc.MIXED_BAD else [])
            for j, es in enumerate(rc.mixed_lists())]


@pytest.fixture(scope="module")
def hot(ctx, oracle_mod):
    return _walked(ctx, oracle_mod, [rc.hot_key_entries()], 1 * MiB)


def _run_relations(ctx, ramcrc, t, relations, what=""):
    """The three adds, with every added batch's live query checked after each
    add (batch 0 after batch 2 included); returns the last answers."""
    ws, exps = relations
    added, got = [], None
    for k, w in enumerate(ws):
        a = tc.Added(w)
        assert a.add(t) == k
        added.append(a)
        got = tc.check_device(ctx, t, added, exps[k], what=(what, "after add", k))
    return added, got


# ------------------------------------------ 1. across batches, every relation
def test_across_batches(ctx, ramcrc, relations):
    ws, exps = relations
    tc.check_relations(ws, exps[2])
    assert exps[0][0][1].shape[0] > exps[2][0][1].shape[0] > 0
    t = ramcrc.ReplayTable(ctx, 2000, 3)
    try:
        added, got = _run_relations(ctx, ramcrc, t, relations)
        _same_as_host(ramcrc, ws, 2000, got, tc.device_stats(ctx, t))
        # without d_winner the list and the counters are the same
        q = tc.Live(ctx, t, added[0], want_winner=False)
        assert q.need == got[0].need and np.array_equal(q.live, got[0].live) and q.counts == got[0].counts
    finally:
        t.close()


# ----------------------------------------------------------------- 2. order
def test_order(ctx, ramcrc, mixed):
    """The four segments of the mixed case as four batches, one of them with a
    bad certificate, in five shuffled add orders on fresh tables: per key the
    surviving (version, type) is the sequential replay's.  In the identity
    order every output equals the device one-call's over the four segments."""
    assert mixed[rc.MIXED_BAD].status[0, 0] & segments.SEG_OK == 0
    want = tc.replayed(mixed)
    assert len(want) > 100
    rng = np.random.default_rng(31)
    for order in [list(range(4))] + [rng.permutation(4).tolist() for _ in range(5)]:
        ws = [mixed[j] for j in order]
        t = ramcrc.ReplayTable(ctx, 1000, 4)
        try:
            added = [tc.Added(w) for w in ws]
            for a in added:
                a.add(t)
            got = tc.check_device(ctx, t, added, tc.expect(ramcrc, ws), what=order)
            assert tc.survivors(ws, [g.live for g in got]) == want, order
            if order == list(range(4)):
                cw = tc.Concat(ws)
                one = rc.Resolved(ctx, cw)
                bounds = np.cumsum([0] + [w.table.shape[0] for w in ws])
                ref = tc.refs(one.winner_all[:bounds[-1]], bounds)
                lives = []
                for j, g in enumerate(got):
                    n = ws[j].table.shape[0]
                    assert np.array_equal(g.winner_all[:n].reshape(-1).view(tc.REF), ref[bounds[j]:bounds[j + 1]])
                    lives.append(g.live[:, 0] + bounds[j])
                assert np.array_equal(np.concatenate(lives), one.live[:, 0])
                assert sum(g.counts["live_objects"] for g in got) == one.counts["live_objects"]
                assert sum(g.counts["objects"] for g in got) == one.counts["objects"]
                assert got[0].counts["safe_version"] == one.counts["safe_version"]
        finally:
            t.close()


# ------------------------------------------------------------ 3. collisions
def test_collisions_across_batches(ctx, ramcrc, oracle_mod):
    """Every caller hash is 7: one probe chain spans both batches, and batch
    1's records read their claimants' keys through batch 0's descriptor."""
    ws = [_walked(ctx, oracle_mod, ls) for ls in tc.split_lists(rc.collision_entries())]
    hs = [np.full(w.table.shape[0], 7, np.uint64) for w in ws]
    t = ramcrc.ReplayTable(ctx, 64, 2)
    try:
        added = [tc.Added(w, h) for w, h in zip(ws, hs)]
        for a in added:
            a.add(t)
        exp = tc.expect(ramcrc, ws, hs)
        got = tc.check_device(ctx, t, added, exp, "hash 7")
        assert tc.device_stats(ctx, t)["keys"] == 50 and exp[1][1].shape[0] > 0
        _same_as_host(ramcrc, ws, 64, got, tc.device_stats(ctx, t), hs)
    finally:
        t.close()


def test_collisions_of_the_seed(ctx, ramcrc, oracle_mod):
    """NULL hashes, table ids 1 and 2^32 + 1 with the same key bytes, split
    over two batches: the computed hashes are equal, the keys stay two."""
    ws = [_walked(ctx, oracle_mod, ls) for ls in tc.split_lists(rc.seed_collision_entries(), at=6)]
    t = ramcrc.ReplayTable(ctx, 64, 2)
    try:
        added = [tc.Added(w) for w in ws]
        for a in added:
            a.add(t)
        tc.check_device(ctx, t, added, tc.expect(ramcrc, ws), "seed")
        assert tc.device_stats(ctx, t)["keys"] == 6
    finally:
        t.close()


def test_given_and_computed_hashes_mix(ctx, ramcrc, mixed):
    """The partition call's d_key_hash for batch 0 and NULL for batch 1:
    identical to NULL for both."""
    ws = mixed[:2]
    tabs = pc.tablets([(tid, 0, tc.ALL, 0, 0, 0) for tid in (1, 2, (1 << 32) + 1)])
    p = pc.Partitioned(ctx, ws[0], tabs, 1, ws[0].table.shape[0] + 8)
    exp = tc.expect(ramcrc, ws)
    outs = []
    for hashes in ((p.d_hash, None), (None, None)):
        t = ramcrc.ReplayTable(ctx, 1000, 2)
        try:
            added = [tc.Added(w, h) for w, h in zip(ws, hashes)]
            for a in added:
                a.add(t)
            outs.append(tc.check_device(ctx, t, added, exp, "given, then computed"))
        finally:
            t.close()
    for a, b in zip(*outs):
        assert np.array_equal(a.winner_all, b.winner_all) and np.array_equal(a.live_all, b.live_all)


# ----------------------------------------------------------- 4. one hot key
def test_one_hot_key(ctx, ramcrc, hot):
    """20,000 records of one key as batch 0, and again as batch 1: every lane
    of both adds meets the one slot."""
    t = ramcrc.ReplayTable(ctx, 8, 2)
    try:
        added = [tc.Added(hot), tc.Added(hot)]
        for a in added:
            a.add(t)
        got = tc.check_device(ctx, t, added, tc.expect(ramcrc, [hot, hot], python=False), "hot")
        assert got[0].live.tolist() == [[19990, 0]] and got[1].need == 0
        assert (got[1].winner_all[:20000] == (0, 19990)).all()
        assert tc.device_stats(ctx, t)["keys"] == 1
    finally:
        t.close()


# ----------------------------------------------------------- 5. small grids
@pytest.fixture(scope="module")
def grid_case(ctx):
    cap = 8 * MiB
    buf, certs, counts = segments.object_segments_host(2, cap, 64)
    w0 = Walked(ctx, buf, certs, cap, 2, min_entry=64)
    w1 = Walked(ctx, buf[:cap].copy(), certs[:1], cap, 1, min_entry=64)
    per = int(counts[0])
    assert per == counts[1] > 80000 and w0.table.shape[0] == 2 * per and w1.table.shape[0] == per
    # the analytic answer: the walk keeps a segment's records together and in
    # offset order, so record k of batch 1 is the twin of segment 0's k-th
    # record in batch 0
    first0 = int(np.flatnonzero(w0.table[:, 0] == 0)[0])
    e0 = np.zeros(2 * per, tc.REF)
    e0["record"] = np.arange(2 * per)
    e1 = np.zeros(per, tc.REF)
    e1["record"] = first0 + np.arange(per)
    live0 = np.arange(2 * per, dtype=np.uint32)
    c0 = dict(objects=2 * per, tombstones=0, live_objects=2 * per, live_tombstones=0, malformed=0,
              safe_version=0)
    c1 = dict(c0, objects=per, live_objects=0)
    exp = [(e0, np.stack([live0, np.zeros_like(live0)], 1), c0), (e1, np.zeros((0, 2), np.uint32), c1)]
    return [w0, w1], exp, 3 * per


@pytest.mark.parametrize("ncu", [0, 1, 3])
def test_small_grids(ramcrc, grid_case, ncu):
    """Batch 0: two 8 MiB segments of 64-byte objects (83,055 records each, all
    keys distinct); batch 1: a byte copy of the first segment.  Every record
    of batch 0 is live, every record of batch 1 has its twin of batch 0 as
    winner.  key_cap is the record count, 249,165, so the table has 524,288
    slots.

    Grids are capped at 8 workgroups of 256 threads per CU.  At 1 CU that is 8
    workgroups, 2,048 threads: k_rtab_insert and k_rtab_pick loop 82 times
    over batch 0's 166,110 records and 41 times over batch 1's;
    k_rtab_tiles and k_rtab_emit take 21 of batch 0's 163 tiles of 1,024 per
    workgroup and 11 of batch 1's 82; k_rtab_stats loops 256 times over the
    slots and k_rtab_zero (the reset before the second round) 1,024 times over
    their 2,097,152 words.  At 3 CUs, 24 workgroups and 6,144 threads: 28 and
    14 passes over the records, 7 and 4 tiles per workgroup, 86 passes over
    the slots and 342 over their words.  k_rtab_scan is one workgroup by
    design (163 tiles in one step of 256) and k_rtab_open one thread.  At the
    default size (256 CUs, 2,048 workgroups) only k_rtab_zero still wraps; 649
    workgroups cover batch 0's records."""
    ws, exp, key_cap = grid_case
    c = ramcrc.Context(0)
    t = None
    try:
        if ncu:
            c.set_cus(ncu)
        t = ramcrc.ReplayTable(c, key_cap, 2)
        for rnd in range(2):
            added = [tc.Added(w) for w in ws]
            for a in added:
                a.add(t)
            got = tc.check_device(c, t, added, exp, what=("grids", ncu, rnd), stats=False)
            st = tc.device_stats(c, t)
            assert st == dict(keys=exp[0][0].shape[0], live_objects=exp[0][0].shape[0], live_tombstones=0,
                              safe_version=0, batches=2, spoiled=0)
            if ncu == 0 and rnd == 0:
                _same_as_host(ramcrc, ws, key_cap, got, st)
            t.reset()
    finally:
        if t is not None:
            t.close()
        c.close()


# ------------------------------------------------- 6. capacity and spoiling
def _spoiled(c, ramcrc, t, added):
    """EREFUSED; live writes only *d_n_live = 0 and zeroed counts; stats only
    spoiled = 1."""
    lives = [tc.Live(c, t, a, check=False) for a in added]
    with pytest.raises(ramcrc.RamcrcError) as e:
        c.check()
    assert e.value.code == ramcrc.EREFUSED
    for r in lives:
        r.read()
        assert r.need == 0 and r.counts == tc.ZERO_COUNTS
        assert (r.live_all == FILL32).all() and (r.winner_all == FILL32).all()
    assert tc.device_stats(c, t) == tc.SPOILED_STATS


def test_capacity_and_spoiling(ramcrc, oracle_mod):
    """key_cap 64 (128 slots): an add that brings the table to exactly 64 keys
    is fine, one more distinct key spoils it until the reset; the same adds on
    a table of key_cap 65 are exact."""
    c = ramcrc.Context(0)
    t = u = None
    try:
        full = _walked(c, oracle_mod, [tc.capacity_lists(64)])
        again = _walked(c, oracle_mod, [tc.capacity_lists(64)[:9]])   # keys the table has
        more = _walked(c, oracle_mod, [[tc.head(2), rc.obj(7, b"one more key", 1)]])
        t = ramcrc.ReplayTable(c, 64, 8)
        added = [tc.Added(full), tc.Added(again)]
        for a in added:
            a.add(t)
        tc.check_device(c, t, added, tc.expect(ramcrc, [full, again]), "exactly key_cap keys")
        assert tc.device_stats(c, t)["keys"] == 64
        added.append(tc.Added(more))
        added[-1].add(t)
        _spoiled(c, ramcrc, t, added)
        # every add until the reset is a no-op on the device: nothing is refused anew
        added.append(tc.Added(again))
        added[-1].add(t)
        c.check()
        assert (added[-1].d_work.view(torch.uint8) == tc.FILL).all()
        lives = [tc.Live(c, t, a) for a in added]
        assert all(r.need == 0 and r.counts == tc.ZERO_COUNTS and (r.live_all == FILL32).all() for r in lives)
        t.reset()
        a = tc.Added(full)
        assert a.add(t) == 0
        tc.check_device(c, t, [a], tc.expect(ramcrc, [full]), "after the reset")
        u = ramcrc.ReplayTable(c, 65, 8)
        added = [tc.Added(w) for w in (full, again, more)]
        for a in added:
            a.add(u)
        tc.check_device(c, u, added, tc.expect(ramcrc, [full, again, more]), "key_cap 65")
        assert tc.device_stats(c, u)["keys"] == 65
    finally:
        for x in (t, u):
            if x is not None:
                x.close()
        c.close()


def test_a_bad_segment_number_spoils(ramcrc, oracle_mod):
    """A record naming segment n_seg spoils the table; reset makes it usable."""
    c = ramcrc.Context(0)
    t = None
    try:
        w = _walked(c, oracle_mod, [[tc.head(1)] + rc.tiny_entries()])
        bad = _walked(c, oracle_mod, [[tc.head(1)] + rc.tiny_entries()])
        bad.d_entries[2, 0] = 1
        t = ramcrc.ReplayTable(c, 64, 4)
        added = [tc.Added(w), tc.Added(bad)]
        for a in added:
            a.add(t)
        _spoiled(c, ramcrc, t, added)
        t.reset()
        a = tc.Added(w)
        a.add(t)
        tc.check_device(c, t, [a], tc.expect(ramcrc, [w]), "after the reset")
    finally:
        if t is not None:
            t.close()
        c.close()


def test_max_batches(ctx, ramcrc, oracle_mod):
    w = _walked(ctx, oracle_mod, [[tc.head(1)] + rc.tiny_entries()])
    t = ramcrc.ReplayTable(ctx, 64, 2)
    try:
        added = [tc.Added(w), tc.Added(w)]
        for a in added:
            a.add(t)
        extra = tc.Added(w)
        with pytest.raises(ramcrc.RamcrcError) as e:
            extra.add(t)
        assert e.value.code == ramcrc.EINVAL
        ctx.check()
        assert (extra.d_work.view(torch.uint8) == tc.FILL).all(), "it launched"
        tc.check_device(ctx, t, added, tc.expect(ramcrc, [w, w]), "still usable")
        z = torch.zeros(16, dtype=torch.int64, device="cuda")
        with pytest.raises(ramcrc.RamcrcError):   # a batch that was never added
            t.live(2, z[8:].view(torch.int32).view(-1, 2), z[6:7], z[:6])
    finally:
        t.close()
    for bad in (0, segments.REPLAY_TABLE_MAX_BATCHES + 1):
        with pytest.raises(ramcrc.RamcrcError):
            ramcrc.ReplayTable(ctx, 64, bad)


# --------------------------------------------------------- 7. list capacity
def _append(c, w, r, out_cap):
    n_out = w.nseg
    out = torch.full((n_out * out_cap,), ac.FILL, dtype=torch.uint8, device="cuda")
    o_certs = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
    o_stat = torch.full((n_out, 2), ac.PATTERN, dtype=torch.int32, device="cuda")
    c.recovery_append(w.d, w.cap, w.nseg, w.d_status, w.d_entries, w.d_n, r.d_live[:r.live_cap],
                      r.d_n_live, 1, out, out_cap, out_cap, o_certs, o_stat)
    return out, o_certs, o_stat


def test_list_capacity(ramcrc, relations):
    """live_cap one less than needed, then 0: the needed count is reported,
    nothing is written past the cap, and the append that follows refuses."""
    ws, exps = relations
    c = ramcrc.Context(0)
    t = ramcrc.ReplayTable(c, 2000, 3)
    try:
        added = [tc.Added(w) for w in ws]
        for a in added:
            a.add(t)
        need = exps[2][1][1].shape[0]
        assert need > 1
        for cap in (need - 1, 0):
            r = tc.check_device(c, t, added[1:2], exps[2][1:2], ("cap", cap), live_cap=cap, stats=False)[0]
            assert r.need == need and r.live.shape[0] == cap
            out, o_certs, _ = _append(c, ws[1], r, ws[1].cap)
            with pytest.raises(ramcrc.RamcrcError) as e:
                c.check()
            assert e.value.code == ramcrc.EREFUSED
            assert (out == ac.FILL).all() and (o_certs == ac.PATTERN).all()
        tc.check_device(c, t, added, exps[2], "after the refused appends")
    finally:
        t.close()
        c.close()


# ----------------------------------------------------------------- 8. state
def test_state(ramcrc, oracle_mod, relations, hot):
    """One table: the relations, reset, the hot key, reset, the relations
    again, with a second table of the same context fed in between; then a
    batch without participants and one without records."""
    ws, exps = relations
    c = ramcrc.Context(0)
    t = ramcrc.ReplayTable(c, 2000, 4)
    u = ramcrc.ReplayTable(c, 2000, 4)
    try:
        added, other = [], []
        for w in ws:   # alternately
            added.append(tc.Added(w))
            added[-1].add(t)
            other.append(tc.Added(hot))
            other[-1].add(u)
        first = tc.check_device(c, t, added, exps[2], "relations")
        tc.check_device(c, u, other, tc.expect(ramcrc, [hot] * 3, python=False), "the other table")
        t.reset()
        a = tc.Added(hot)
        a.add(t)
        tc.check_device(c, t, [a], tc.expect(ramcrc, [hot], python=False), "hot")
        t.reset()
        _, second = _run_relations(c, ramcrc, t, relations, "again")
        for x, y in zip(first, second):
            assert np.array_equal(x.winner_all, y.winner_all) and np.array_equal(x.live_all, y.live_all)
            assert x.counts == y.counts
        tc.check_device(c, u, other, tc.expect(ramcrc, [hot] * 3, python=False), "the other table, after")
        quiet = _walked(c, oracle_mod, [[tc.head(3), pc.entry(pc.LOGDIGEST, b"d")]])
        empty = _walked(c, oracle_mod, [[tc.head(3), pc.entry(pc.LOGDIGEST, b"d")]])
        empty.d_n.zero_()
        empty.table = empty.table[:0]
        t.reset()
        added = [tc.Added(w) for w in (quiet, ws[0], empty)]
        for a in added:
            a.add(t)
        got = tc.check_device(c, t, added, tc.expect(ramcrc, [quiet, ws[0], empty]), "quiet, 0, empty")
        assert (got[0].winner_all[:2] == tc.NONE).all() and (got[2].winner_all == FILL32).all()
    finally:
        t.close()
        u.close()
        c.close()


# ----------------------------------------------------------------- 9. chain
def test_chain(ctx, ramcrc, oracle_mod, mixed):
    """Two batches of two segments: walk -> verify -> add -> add -> live(0),
    live(1) -> append with n_part = 1 per batch.  The outputs equal
    ramcrc_recovery_append_host over the host table's lists byte for byte,
    pass a device walk with RAMCRC_SEG_OK, and hold, per batch, exactly the
    records the one-call resolve of the concatenation keeps."""
    lists = rc.mixed_lists()
    ws = [_walked(ctx, oracle_mod, lists[:2], rc.MIXED_CAP), _walked(ctx, oracle_mod, lists[2:], rc.MIXED_CAP)]
    exp = tc.expect(ramcrc, ws)
    t = ramcrc.ReplayTable(ctx, 1000, 2)
    try:
        added = []
        for w in ws:
            crc = torch.zeros(w.d_entries.shape[0], dtype=torch.int32, device="cuda")
            ctx.verify_objects(w.d, w.cap, w.d_entries, w.d_n, crc, w.d_status.clone())
            added.append(tc.Added(w))
            added[-1].add(t)
        lives = [tc.Live(ctx, t, a, check=False) for a in added]
        outs = [_append(ctx, w, r, w.cap) for w, r in zip(ws, lives)]
        ctx.check()
        host, _ = _host_table(ramcrc, ws, 1000)
        for j, (w, r, (out, o_certs, o_stat)) in enumerate(zip(ws, lives, outs)):
            r.read()
            h_live = host[j][1]
            assert np.array_equal(r.live, exp[j][1]) and np.array_equal(h_live, r.live) and r.need > 20
            h_out = np.full(w.nseg * w.cap, ac.FILL, np.uint8)
            h_certs, h_stat = ramcrc.recovery_append_host(w.buf, w.cap, w.nseg, w.status, w.table, h_live,
                                                          1, h_out, w.cap, w.cap)
            got = out.cpu().numpy()
            assert np.array_equal(got, h_out), "bytes"
            assert np.array_equal(_u32(o_certs), h_certs) and np.array_equal(_u32(o_stat), h_stat)
            w2 = Walked(ctx, got, _u32(o_certs), w.cap, w.nseg, d_buf=out)
            assert (w2.status[:, 0] == segments.SEG_OK).all()
            for s in range(w.nseg):
                src = w.table[r.live[:, 0]]
                src = src[src[:, 0] == s]
                dst = w2.table[w2.table[:, 0] == s]
                assert dst.shape[0] == src.shape[0] == _u32(o_stat)[s, 1] > 0
                assert np.array_equal(dst[:, 2], src[:, 2]) and np.array_equal(dst[:, 3] & 0x3F, src[:, 3] & 0x3F)
    finally:
        t.close()


# ---------------------------------------------------- 10. reference scenarios
def test_reference_scenarios(ctx, ramcrc, oracle_mod):
    ref = pc.load("replay_resolve_ref.json")
    lists, which = tc.reference_lists(ref)
    ws = [_walked(ctx, oracle_mod, [es]) for es in lists]
    t = ramcrc.ReplayTable(ctx, 256, len(ws))
    try:
        added = [tc.Added(w) for w in ws]
        for a in added:
            a.add(t)
        exp = tc.expect(ramcrc, ws)
        tc.check_device(ctx, t, added, exp, "reference")
        tc.check_reference(ref, which, exp, ws)
    finally:
        t.close()
